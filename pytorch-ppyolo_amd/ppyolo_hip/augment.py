"""Training batches on the device: the reference's training reader (train.py:36-152 with the transforms of
config/ppyolo_2x.py:154-251), restated as a host PLANNER plus two HIP kernels (csrc/augment.hip).

    DecodeImage -> MixupImage -> ColorDistort -> RandomExpand -> RandomCrop -> RandomFlipImage -> NormalizeBox -> PadBox
    -> BboxXYXY2XYWH -> RandomShapeSingle -> NormalizeImage -> Permute -> Gt2YoloTargetSingle

The planner makes every random decision and all box arithmetic on the host, in numpy, operation for operation as the
reference's classes (tools/transform.py) make them.  It never touches a pixel: per sample it produces a small RECIPE
(mixup factor, colour ops and their constants, expand canvas, crop window, flip, interpolation and its coefficient tables,
the image's dtype at each stage) and the final padded boxes.  The render kernel evaluates the pre-resize image of a
recipe straight from the uint8 sources and resizes / normalises it into NCHW float32; the target kernel writes the dense
YOLO targets from per-box records that `targets.gt2yolo_records` computes with `targets.gt2yolo_target`'s arithmetic.

DRAW ORDER.  With `rng` = np.random (the default) the planner consumes exactly the draws the reference's
`multi_thread_op` makes with cfg.train_cfg num_threads = 1, in the same order: for each sample in batch order, all
sample transforms, then that sample's RandomShapeSingle interpolation draw.  (With more threads the reference's own
order is nondeterministic: all its threads share the global np.random.)  The batch's `shape` is drawn by the caller
before get_samples, as train.py:90 does.

SOURCES.  A record's image (and its mixup partner's) is a numpy array, a CPU tensor -- both are packed into the blob -- or a
uint8 [h,w,3] tensor on the builder's device with pixel stride 3 (what JpegDecoder returns, or a cropped view of a larger
tensor): the kernels read that one where it lies, no pixel of it visits the host.  `decode_records` / `from_files` are the
reference's DecodeImage on the device: records with 'im_file' or JPEG bytes in, device-resident images out.

Settings the reference configs do not use are refused with PPYoloHipError (cutmix, hsv_format, random_channel,
random_apply=False, resize_box, mask / keypoint fields, a dsize that is not shape x shape).
"""
import re

import numpy as np
import torch

from . import ops, targets
from ._lib import PPYoloHipError
from .hostio import check_image
from .preprocess import normalisation_table

NEAREST, LINEAR, CUBIC, AREA, LANCZOS4 = 0, 1, 2, 3, 4        # cv2.INTER_* codes
INTERPS = [NEAREST, LINEAR, AREA, CUBIC, LANCZOS4]          # RandomShapeSingle.interps, in the reference's order
U8, F32, F64 = 0, 1, 2                                      # image dtypes of the chain
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
# resize modes of the render kernel (csrc/augment.hip): index map / separable tables / integer-scale area
MODE_NEAREST, MODE_SEP, MODE_AREA_FAST = 0, 1, 2
FIELDS = ['image', 'gt_bbox', 'gt_class', 'gt_score']       # the builder's own context field list
_DBL_EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------------------------------
# OpenCV 4.x resize coefficient tables (imgproc/src/resize.cpp), one axis at a time.  The kernel clamps every tap index to
# the source extent (replicated border) and applies the weights; fixed point (uint8 generic) keeps int16 weights exactly.

def _cubic(x):
    """interpolateCubic, float32 operation by operation (x: float32 array) -> [n, 4]."""
    f = np.float32
    A = f(-0.75)
    t = x + f(1)
    c0 = ((A * t - f(5) * A) * t + f(8) * A) * t - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    u = f(1) - x
    c2 = ((A + f(2)) * u - (A + f(3))) * u * u + f(1)
    c3 = f(1) - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.float32)


_S45 = 0.70710678118654752440084436210485
_LCS = [(1, 0), (-_S45, -_S45), (0, 1), (_S45, -_S45), (-1, 0), (_S45, _S45), (0, -1), (-_S45, _S45)]


def _lanczos4(x):
    """interpolateLanczos4 (x: float32 array) -> [n, 8]: float64 sin / cos of the float32 argument, coefficients rounded to
    float32, summed in float32 in tap order, scaled by the float32 reciprocal; x < FLT_EPSILON gives the unit tap."""
    f = np.float32
    y0 = (-(x + f(3))).astype(np.float64) * np.pi * 0.25
    s0, c0 = np.sin(y0), np.cos(y0)
    c = np.empty(x.shape + (8,), np.float32)
    s = np.zeros(x.shape, np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(8):
            y = (-(x + f(3) - f(i))).astype(np.float64) * np.pi * 0.25
            c[:, i] = ((_LCS[i][0] * s0 + _LCS[i][1] * c0) / (y * y)).astype(np.float32)
            s = s + c[:, i]
        c = c * (f(1) / s)[:, None]
    small = x < np.finfo(np.float32).eps
    c[small] = 0
    c[small, 3] = 1
    return c


def _generic_table(interp, n_src, n_dst, inv_scale, fixpt):
    """resizeGeneric's xofs / alpha (or yofs / beta) for one axis -> (first tap int32 [n_dst], weights float32 [n_dst, K])."""
    scale = 1.0 / inv_scale
    K = {LINEAR: 2, AREA: 2, CUBIC: 4, LANCZOS4: 8}[interp]
    d = np.arange(n_dst, dtype=np.float64)
    if interp != AREA:
        f = ((d + 0.5) * scale - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(np.float32)).astype(np.float32)
    else:                                                   # area_mode: the upscaling emulation of INTER_AREA
        s = np.floor(d * scale).astype(np.int64)
        f = ((d + 1) - (s + 1) * inv_scale).astype(np.float32)
        f = np.where(f <= 0, np.float32(0), (f - np.floor(f).astype(np.float32)).astype(np.float32))
    if interp in (LINEAR, AREA):
        lo, hi = s < 0, s >= n_src - 1
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
        s = np.where(lo, 0, np.where(hi, n_src - 1, s))
        c = np.stack([np.float32(1) - f, f], axis=-1).astype(np.float32)
    elif interp == CUBIC:
        c = _cubic(f)
    else:
        c = _lanczos4(f)
    first = (s - (K // 2 - 1)).astype(np.int32)
    if fixpt:
        c = np.clip(np.rint(c * np.float32(2048)), -32768, 32767).astype(np.float32)
    return first, np.ascontiguousarray(c, dtype=np.float32)


def _area_table(n_src, n_dst, scale):
    """computeResizeAreaTab, entries of one destination index padded with zero weights to the widest."""
    rows = []
    for d in range(n_dst):
        fs1 = d * scale
        fs2 = fs1 + scale
        cell = min(scale, n_src - fs1)
        s1, s2 = int(np.ceil(fs1)), int(np.floor(fs2))
        s2 = min(s2, n_src - 1)
        s1 = min(s1, s2)
        ent = []
        if s1 - fs1 > 1e-3:
            ent.append((s1 - 1, np.float32((s1 - fs1) / cell)))
        for s in range(s1, s2):
            ent.append((s, np.float32(1.0 / cell)))
        if fs2 - s2 > 1e-3:
            ent.append((s2, np.float32(min(min(fs2 - s2, 1.), cell) / cell)))
        rows.append(ent)
    K = max(len(e) for e in rows)
    first = np.array([e[0][0] for e in rows], np.int32)
    w = np.zeros((n_dst, K), np.float32)
    for d, ent in enumerate(rows):
        for k, (s, a) in enumerate(ent):
            assert s == first[d] + k
            w[d, k] = a
    return first, w


def resize_plan(h, w, fx, fy, interp, dtype):
    """cv2.resize(canvas [h,w,3] of `dtype`, None, fx=fx, fy=fy, interpolation=interp) as the render kernel runs it:
    dict(mode, fixpt, xfirst, xw, yfirst, yw, ix, iy).  Raises when cv2's dsize would not be a square of the batch."""
    dw, dh = int(np.rint(w * fx)), int(np.rint(h * fy))
    plan = dict(dw=dw, dh=dh, fixpt=0, ix=0, iy=0)
    scale_x, scale_y = 1.0 / fx, 1.0 / fy
    if dw == w and dh == h:                                            # cv::resize: dsize == ssize -> copyTo
        interp = NEAREST
    if interp == NEAREST:
        plan.update(mode=MODE_NEAREST,
                    xfirst=np.minimum(np.floor(np.arange(dw) * scale_x).astype(np.int64), w - 1).astype(np.int32),
                    yfirst=np.minimum(np.floor(np.arange(dh) * scale_y).astype(np.int64), h - 1).astype(np.int32),
                    xw=np.ones((dw, 1), np.float32), yw=np.ones((dh, 1), np.float32))
        return plan
    ix, iy = int(np.rint(scale_x)), int(np.rint(scale_y))
    area_fast = abs(scale_x - ix) < _DBL_EPS and abs(scale_y - iy) < _DBL_EPS
    if interp == LINEAR and area_fast and ix == 2 and iy == 2:
        interp = AREA
    if interp == AREA and scale_x >= 1 and scale_y >= 1:
        if area_fast:
            plan.update(mode=MODE_AREA_FAST, ix=ix, iy=iy, xfirst=(np.arange(dw) * ix).astype(np.int32),
                        yfirst=(np.arange(dh) * iy).astype(np.int32), xw=np.ones((dw, 1), np.float32),
                        yw=np.ones((dh, 1), np.float32))
            return plan
        xf, xw = _area_table(w, dw, scale_x)
        yf, yw = _area_table(h, dh, scale_y)
        plan.update(mode=MODE_SEP, xfirst=xf, xw=xw, yfirst=yf, yw=yw)
        return plan
    fixpt = int(dtype == U8)
    xf, xw = _generic_table(interp, w, dw, fx, fixpt)
    yf, yw = _generic_table(interp, h, dh, fy, fixpt)
    plan.update(mode=MODE_SEP, fixpt=fixpt, xfirst=xf, xw=xw, yfirst=yf, yw=yw)
    return plan


# ---------------------------------------------------------------------------------------------------------------------

def _hue_matrix(delta):
    u = np.cos(delta * np.pi)
    w = np.sin(delta * np.pi)
    bt = np.array([[1.0, 0.0, 0.0], [0.0, u, -w], [0.0, w, u]])
    tyiq = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.321], [0.211, -0.523, 0.311]])
    ityiq = np.array([[1.0, 0.956, 0.621], [1.0, -0.272, -0.647], [1.0, -1.107, 1.705]])
    return np.dot(np.dot(ityiq, bt), tyiq).T


def _iou_matrix(a, b):
    tl_i = np.maximum(a[:, np.newaxis, :2], b[:, :2])
    br_i = np.minimum(a[:, np.newaxis, 2:], b[:, 2:])
    area_i = np.prod(br_i - tl_i, axis=2) * (tl_i < br_i).all(axis=2)
    area_a = np.prod(a[:, 2:] - a[:, :2], axis=1)
    area_b = np.prod(b[:, 2:] - b[:, :2], axis=1)
    area_o = (area_a[:, np.newaxis] + area_b - area_i)
    return area_i / (area_o + 1e-10)


def _crop_boxes(box, crop):
    cropped = box.copy()
    cropped[:, :2] = np.maximum(box[:, :2], crop[:2])
    cropped[:, 2:] = np.minimum(box[:, 2:], crop[2:])
    cropped[:, :2] -= crop[:2]
    cropped[:, 2:] -= crop[:2]
    centers = (box[:, :2] + box[:, 2:]) / 2
    valid = np.logical_and(crop[:2] <= centers, centers < crop[2:]).all(axis=1)
    valid = np.logical_and(valid, (cropped[:, :2] < cropped[:, 2:]).all(axis=1))
    return cropped, np.where(valid)[0]


class TrainBatchBuilder(object):
    """cfg-driven training batches: `builder(samples, shape)` -> the batch dict of the reference's read_train_data
    (train.py:80-88) on the device: images float32 [N,3,S,S], gt_bbox float32 [N,50,4], gt_class int32 [N,50],
    gt_score float32 [N,50], target0..L-1 float32 [N,3,6+C,S/ds,S/ds].  `samples` are records after DecodeImage with
    the image as cv2.imdecode gives it (uint8 HWC BGR): image, h, w, gt_bbox [G,4] xyxy px float32, gt_class [G,1]
    int32, gt_score [G,1] float32, is_crowd, optional `mixup` sub-record of the same form.  `image` may also be a tensor:
    see `source_image`."""

    def __init__(self, cfg, device='cuda'):
        self.device = torch.device(device)
        d = cfg.decodeImage
        if d.get('with_cutmix', False):
            raise PPYoloHipError('cutmix is not implemented (the reference configs do not use it)')
        self.to_rgb = bool(d['to_rgb'])
        self.with_mixup = bool(d.get('with_mixup', False))
        self.mix_a, self.mix_b = cfg.mixupImage.get('alpha', 1.5), cfg.mixupImage.get('beta', 1.5)
        cd = dict(hue=[-18, 18, 0.5], saturation=[0.5, 1.5, 0.5], contrast=[0.5, 1.5, 0.5], brightness=[0.5, 1.5, 0.5],
                  random_apply=True, hsv_format=False, random_channel=False)
        cd.update(cfg.colorDistort)
        if cd['hsv_format'] or cd['random_channel'] or not cd['random_apply']:
            raise PPYoloHipError('ColorDistort: only random_apply=True without hsv_format / random_channel is implemented')
        self.cd = cd
        ex = dict(ratio=4., prob=0.5, fill_value=(127.5,) * 3, is_mask_expand=False)
        ex.update(cfg.randomExpand)
        if ex['is_mask_expand']:
            raise PPYoloHipError('RandomExpand: mask fields are not implemented')
        fv = ex['fill_value']
        fv = (fv,) * 3 if np.isscalar(fv) else tuple(fv)
        self.expand_ratio, self.expand_prob = ex['ratio'], ex['prob']
        self.fill = np.array(fv, dtype=np.uint8)           # as the reference's canvas *= np.array(fill, uint8)
        rc = dict(aspect_ratio=[.5, 2.], thresholds=[.0, .1, .3, .5, .7, .9], scaling=[.3, 1.], num_attempts=50,
                  allow_no_crop=True, cover_all_box=False, is_mask_crop=False)
        rc.update(cfg.randomCrop)
        if rc['is_mask_crop']:
            raise PPYoloHipError('RandomCrop: mask fields are not implemented')
        self.rc = rc
        fl = dict(prob=0.5, is_normalized=False, is_mask_flip=False)
        fl.update(cfg.randomFlipImage)
        if fl['is_mask_flip']:
            raise PPYoloHipError('RandomFlipImage: mask fields are not implemented')
        self.flip_prob, self.flip_normalized = fl['prob'], fl['is_normalized']
        self.num_max_boxes = cfg.padBox.get('num_max_boxes', 50)
        rs = cfg.randomShape
        if rs.get('resize_box', False):
            raise PPYoloHipError('RandomShape: resize_box is not implemented')
        self.random_inter = bool(rs.get('random_inter', False))
        self.sample_seq = list(cfg.sample_transforms_seq)
        self.batch_seq = list(cfg.batch_transforms_seq)
        known = ['decodeImage', 'mixupImage', 'colorDistort', 'randomExpand', 'randomCrop', 'randomFlipImage',
                 'normalizeBox', 'padBox', 'bboxXYXY2XYWH']
        if [s for s in self.sample_seq if s not in known] or self.batch_seq != ['randomShape', 'normalizeImage', 'permute', 'gt2YoloTarget']:
            raise PPYoloHipError('unsupported transform sequence %s / %s' % (self.sample_seq, self.batch_seq))
        n = cfg.normalizeImage
        if n.get('is_channel_first', False) or not cfg.permute.get('channel_first', True) or cfg.permute.get('to_bgr', False):
            raise PPYoloHipError('only the reference training layout is implemented: HWC normalise, CHW output, RGB')
        self.mean, self.std, self.is_scale = list(n['mean']), list(n['std']), bool(n.get('is_scale', True))
        self.lut_np = normalisation_table(self.mean, self.std, self.is_scale)
        g = cfg.gt2YoloTarget
        self.anchors, self.anchor_masks = g['anchors'], g['anchor_masks']
        self.downsample_ratios, self.num_classes = g['downsample_ratios'], g['num_classes']
        self.iou_thresh = g.get('iou_thresh', 1.)
        self._lut = None
        self._decoder = None

    # ---------------------------------------------------------------------------------------------------------------
    # one sample, transform by transform (the reference's classes, draw for draw; images are only their extents)

    def _mixup(self, s, rng):
        if 'mixup' not in s:
            return s
        factor = rng.beta(self.mix_a, self.mix_b)
        factor = max(0.0, min(1.0, factor))
        if factor >= 1.0:
            s.pop('mixup')
            return s
        if factor <= 0.0:
            return s['mixup']
        m = s.pop('mixup')
        s['mix'] = dict(factor=factor, image=m['image'])
        s['gt_bbox'] = np.concatenate((s['gt_bbox'], m['gt_bbox']), axis=0)
        s['gt_class'] = np.concatenate((s['gt_class'], m['gt_class']), axis=0)
        s['gt_score'] = np.concatenate((s['gt_score'] * factor, m['gt_score'] * (1. - factor)), axis=0)
        s['is_crowd'] = np.concatenate((s['is_crowd'], m['is_crowd']), axis=0)
        s['h'] = max(s['h'], m['image'].shape[0])
        s['w'] = max(s['w'], m['image'].shape[1])
        return s

    def _color(self, s, rng):
        ops_ = rng.permutation(['brightness', 'contrast', 'saturation', 'hue'])
        for name in ops_:
            low, high, prob = self.cd[str(name)]
            if rng.uniform(0., 1.) < prob:
                continue
            delta = rng.uniform(low, high)
            if name == 'hue':
                s['ops'].append((OP_HUE, delta, _hue_matrix(delta)))
            else:
                s['ops'].append(({'brightness': OP_BRIGHTNESS, 'contrast': OP_CONTRAST, 'saturation': OP_SATURATION}[str(name)],
                                 delta, None))
        return s

    def _expand(self, s, rng):
        if rng.uniform(0., 1.) < self.expand_prob:
            return s
        height, width = int(s['h']), int(s['w'])
        ratio = rng.uniform(1., self.expand_ratio)
        h, w = int(height * ratio), int(width * ratio)
        if not h > height or not w > width:
            return s
        y = rng.randint(0, h - height)
        x = rng.randint(0, w - width)
        s['expand'] = (h, w, y, x)
        s['h'], s['w'] = h, w
        if len(s['gt_bbox']) > 0:
            s['gt_bbox'] += np.array([x, y] * 2, dtype=np.float32)
        return s

    def _crop(self, s, rng):
        if len(s['gt_bbox']) == 0:
            return s
        h, w, gt_bbox, rc = s['h'], s['w'], s['gt_bbox'], self.rc
        thresholds = list(rc['thresholds'])
        if rc['allow_no_crop']:
            thresholds.append('no_crop')
        rng.shuffle(thresholds)
        for thresh in thresholds:
            if thresh == 'no_crop':
                return s
            found = False
            for _ in range(rc['num_attempts']):
                scale = rng.uniform(*rc['scaling'])
                if rc['aspect_ratio'] is not None:
                    min_ar, max_ar = rc['aspect_ratio']
                    ar = rng.uniform(max(min_ar, scale ** 2), min(max_ar, scale ** -2))
                    h_scale, w_scale = scale / np.sqrt(ar), scale * np.sqrt(ar)
                else:
                    h_scale, w_scale = rng.uniform(*rc['scaling']), rng.uniform(*rc['scaling'])
                crop_h, crop_w = h * h_scale, w * w_scale
                if rc['aspect_ratio'] is None and (crop_h / crop_w < 0.5 or crop_h / crop_w > 2.0):
                    continue
                crop_h, crop_w = int(crop_h), int(crop_w)
                crop_y = rng.randint(0, h - crop_h)
                crop_x = rng.randint(0, w - crop_w)
                crop_box = [crop_x, crop_y, crop_x + crop_w, crop_y + crop_h]
                iou = _iou_matrix(gt_bbox, np.array([crop_box], dtype=np.float32))
                if iou.max() < thresh:
                    continue
                if rc['cover_all_box'] and iou.min() < thresh:
                    continue
                cropped, valid = _crop_boxes(gt_bbox, np.array(crop_box, dtype=np.float32))
                if valid.size > 0:
                    found = True
                    break
            if found:
                x1, y1, x2, y2 = crop_box
                cy, cx, _, _ = s['crop']
                s['crop'] = (cy + y1, cx + x1, y2 - y1, x2 - x1)
                s['gt_bbox'] = np.take(cropped, valid, axis=0)
                s['gt_class'] = np.take(s['gt_class'], valid, axis=0)
                s['w'], s['h'] = x2 - x1, y2 - y1
                s['gt_score'] = np.take(s['gt_score'], valid, axis=0)
                s['is_crowd'] = np.take(s['is_crowd'], valid, axis=0)
                return s
        return s

    def _flip(self, s, rng):
        gt_bbox = s['gt_bbox']
        width = s['crop'][3]
        if rng.uniform(0, 1) < self.flip_prob:
            if gt_bbox.shape[0] == 0:
                return s                                    # the reference returns before the image is flipped
            oldx1, oldx2 = gt_bbox[:, 0].copy(), gt_bbox[:, 2].copy()
            if self.flip_normalized:
                gt_bbox[:, 0], gt_bbox[:, 2] = 1 - oldx2, 1 - oldx1
            else:
                gt_bbox[:, 0] = width - oldx2 - 1
                gt_bbox[:, 2] = width - oldx1 - 1
            if gt_bbox.shape[0] != 0 and (gt_bbox[:, 2] < gt_bbox[:, 0]).all():
                raise PPYoloHipError('RandomFlipImage: invalid box, x2 should be greater than x1')
            s['gt_bbox'] = gt_bbox
            s['flip'] = True
        return s

    def _normalize_box(self, s):
        gt_bbox, width, height = s['gt_bbox'], s['w'], s['h']
        for i in range(gt_bbox.shape[0]):
            gt_bbox[i][0] = gt_bbox[i][0] / width
            gt_bbox[i][1] = gt_bbox[i][1] / height
            gt_bbox[i][2] = gt_bbox[i][2] / width
            gt_bbox[i][3] = gt_bbox[i][3] / height
        return s

    def _pad_box(self, s):
        bbox, num_max = s['gt_bbox'], self.num_max_boxes
        gt_num = min(num_max, len(bbox))
        pad_bbox = np.zeros((num_max, 4), dtype=np.float32)
        pad_class = np.zeros((num_max), dtype=np.int32)
        pad_score = np.zeros((num_max), dtype=np.float32)
        if gt_num > 0:
            pad_bbox[:gt_num, :] = bbox[:gt_num, :]
            pad_class[:gt_num] = s['gt_class'][:gt_num, 0]
            pad_score[:gt_num] = s['gt_score'][:gt_num, 0]
        s['gt_bbox'], s['gt_class'], s['gt_score'] = pad_bbox, pad_class, pad_score
        return s

    @staticmethod
    def _xyxy2xywh(s):
        bbox = s['gt_bbox']
        bbox[:, 2:4] = bbox[:, 2:4] - bbox[:, :2]
        bbox[:, :2] = bbox[:, :2] + bbox[:, 2:4] / 2.
        return s

    def _check_record(self, rec):
        for k in ('gt_poly', 'gt_keypoint', 'cutmix', 'semantic'):
            if rec.get(k) is not None:
                raise PPYoloHipError('field %r is not implemented (the reference configs do not use it)' % k)
        return source_image(rec['image'], self.device)

    @staticmethod
    def _fresh(rec, image):
        """A record as DecodeImage leaves it, plus the planner's image state (no pixel is touched)."""
        s = dict(rec, image=image)
        for k in ('gt_bbox', 'gt_class', 'gt_score', 'is_crowd'):
            s[k] = np.array(rec[k], copy=True)
        s['h'], s['w'] = (int(v) for v in image.shape[:2])  # DecodeImage: h / w from the decoded image
        s.update(ops=[], mix=None, expand=None, flip=False, crop=(0, 0, s['h'], s['w']))
        return s

    def _plan_one(self, rec, shape, rng):
        s = self._fresh(rec, self._check_record(rec))
        if 'mixup' in rec:
            if self.with_mixup:
                s['mixup'] = self._fresh(rec['mixup'], self._check_record(rec['mixup']))
            else:
                s.pop('mixup')
        for name in self.sample_seq:
            if name == 'mixupImage':
                if self.with_mixup:
                    s = self._mixup(s, rng)
                    s['crop'] = (0, 0, s['h'], s['w'])
            elif name == 'colorDistort':
                s = self._color(s, rng)
            elif name == 'randomExpand':
                s = self._expand(s, rng)
                s['crop'] = (0, 0, s['h'], s['w'])
            elif name == 'randomCrop':
                s = self._crop(s, rng)
            elif name == 'randomFlipImage':
                s = self._flip(s, rng)
            elif name == 'normalizeBox':
                s = self._normalize_box(s)
            elif name == 'padBox':
                s = self._pad_box(s)
            elif name == 'bboxXYXY2XYWH':
                s = self._xyxy2xywh(s)
        interp = rng.choice(INTERPS) if self.random_inter else NEAREST
        ch, cw = s['crop'][2], s['crop'][3]
        fx, fy = float(shape) / cw, float(shape) / ch
        color_dtype = _color_dtype(s['ops'])
        canvas_dtype = U8 if s['expand'] is not None else color_dtype
        rp = resize_plan(ch, cw, fx, fy, int(interp), canvas_dtype)
        if rp['dw'] != shape or rp['dh'] != shape:
            raise PPYoloHipError('cv2.resize would give %dx%d, not %dx%d (the reference fails there as well)'
                                 % (rp['dw'], rp['dh'], shape, shape))
        mix = s['mix']
        recipe = dict(image=s['image'], mix_image=None if mix is None else mix['image'],
                      factor=None if mix is None else mix['factor'], ops=s['ops'], color_dtype=color_dtype,
                      expand=s['expand'], fill=self.fill, crop=s['crop'], flip=bool(s['flip']),
                      canvas_dtype=canvas_dtype, interp=int(interp), fx=fx, fy=fy, resize=rp)
        return recipe, s['gt_bbox'], s['gt_class'], s['gt_score']

    def plan(self, samples, shape, rng=np.random):
        """Host half, no GPU: (recipes, gt_bbox float32 [N,50,4], gt_class int32 [N,50], gt_score float32 [N,50])."""
        shape = int(shape)
        recipes, bb, cl, sc = [], [], [], []
        for rec in samples:
            r, b, c, s = self._plan_one(rec, shape, rng)
            recipes.append(r)
            bb.append(b)
            cl.append(c)
            sc.append(s)
        return recipes, np.stack(bb), np.stack(cl), np.stack(sc)

    # ---------------------------------------------------------------------------------------------------------------

    def __call__(self, samples, shape, rng=np.random):
        shape = int(shape)
        recipes, gt_bbox, gt_class, gt_score = self.plan(samples, shape, rng)
        N = len(recipes)
        levels = [int(shape / ds) for ds in self.downsample_ratios]
        offs, vals = targets.gt2yolo_records(gt_bbox, gt_class, gt_score, self.anchors, self.anchor_masks,
                                             self.downsample_ratios, self.num_classes, shape, self.iou_thresh)
        blob, layout = pack_batch(recipes, self.to_rgb, offs, vals, gt_bbox, gt_class, gt_score)
        pinned = torch.from_numpy(blob).pin_memory()
        dev = pinned.to(self.device, non_blocking=True)
        if self._lut is None:
            self._lut = torch.from_numpy(self.lut_np).to(self.device)
        images = torch.empty((N, 3, shape, shape), dtype=torch.float32, device=self.device)
        sizes = [N * len(m) * (6 + self.num_classes) * g * g for m, g in zip(self.anchor_masks, levels)]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        sources = self._hold(layout['sources'])
        ops.augment_render(dev, N, shape, self._lut, self.mean, self.std, images, self.is_scale, sources=sources)
        ops.augment_targets(flat, dev, layout['toff'], layout['tval'], len(offs))
        self._keep = (pinned, dev, sources)         # (the blob's boxes are views into dev; the launch reads the sources)
        out = dict(images=images)
        box = dev[layout['gt_bbox']:layout['gt_bbox'] + gt_bbox.nbytes].view(torch.float32).view(N, -1, 4)
        out['gt_bbox'] = box
        out['gt_class'] = dev[layout['gt_class']:layout['gt_class'] + gt_class.nbytes].view(torch.int32).view(N, -1)
        out['gt_score'] = dev[layout['gt_score']:layout['gt_score'] + gt_score.nbytes].view(torch.float32).view(N, -1)
        o = 0
        for i, (m, g) in enumerate(zip(self.anchor_masks, levels)):
            out['target%d' % i] = flat[o:o + sizes[i]].view(N, len(m), 6 + self.num_classes, g, g)
            o += sizes[i]
        return out

    def canvas(self, recipe, to_rgb=None):
        """Debug: the pre-resize image of one planned sample, from the device, in its natural dtype [h, w, 3]."""
        blob, layout = pack_batch([recipe], self.to_rgb if to_rgb is None else to_rgb, np.zeros(0, np.int64),
                                  np.zeros(0, np.float32), None, None, None)
        dev = torch.from_numpy(blob).pin_memory().to(self.device, non_blocking=True)
        ch, cw = recipe['crop'][2], recipe['crop'][3]
        dt = {U8: torch.uint8, F32: torch.float32, F64: torch.float64}[recipe['canvas_dtype']]
        out = torch.empty((ch, cw, 3), dtype=dt, device=self.device)
        ops.augment_canvas(dev, 0, out, sources=self._hold(layout['sources']))
        return out

    def _hold(self, sources):
        """External sources are read by launches on the current stream: tell the allocator, so that memory a caller drops
        right after the call (or that another stream's decoder owns) is not handed out again under the kernel."""
        if sources:
            cur = torch.cuda.current_stream(self.device)
            for t in sources:
                t.record_stream(cur)
        return sources

    def from_files(self, records, shape, rng=np.random, decoder=None, fallback=None):
        """`builder(decode_records(records), shape, rng)`: records carry 'im_file' (or JPEG bytes as 'image'), as the
        reference's do before DecodeImage; every file of the batch goes through one decoder.decode() call (default: a
        JpegDecoder the builder owns, checked decode) and stays on the device.  fallback: see decode_records."""
        if decoder is None:
            if self._decoder is None:
                from .jpeg import JpegDecoder
                self._decoder = JpegDecoder(device=self.device)
            decoder = self._decoder
        return self(decode_records(records, decoder, fallback, with_mixup=self.with_mixup), shape, rng)


def source_image(im, device):
    """What the builder makes of a record's image: a numpy uint8 [h,w,3] array (as given, or the one a CPU tensor wraps) is a
    HOST source, packed into the blob; a uint8 [h,w,3] tensor on `device` under hostio.check_image's rule is returned as it
    is, an EXTERNAL source the kernels read in place.  Anything else raises: nothing is copied silently."""
    if isinstance(im, torch.Tensor):
        check_image(None, im, device, 'source', host=True)
        return im.numpy() if im.device.type == 'cpu' else im
    if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
        raise PPYoloHipError('expected a decoded uint8 image [h, w, 3]')
    return im


def is_external(im):
    """pack_batch's rule: a tensor that is not in host memory stays where it is."""
    return isinstance(im, torch.Tensor) and im.device.type != 'cpu'


def decode_records(records, decoder=None, fallback=None, with_mixup=True):
    """The reference's DecodeImage.__call__ (tools/transform.py:79-128) for a whole batch, without the colour swap (the render
    kernel's to_rgb does it): a record is decoded if it has no 'image' (its 'im_file' is read) or if its 'image' is bytes; so
    is its 'mixup' record when with_mixup is set.  All of them go through ONE decoder.decode([bytes, ...]) call; 'image'
    becomes the tensor it returns and 'h' / 'w' are set from it.  Records (and mixup records) are shallow copies: the
    caller's list is not changed.

    decoder: an object with decode(list of bytes) -> list of uint8 [h,w,3] BGR tensors, default JpegDecoder().  If it has
    refusal(bytes) -> None | (kind, reason) (JpegDecoder: a header-only pass), the files it would refuse are found before
    anything is decoded.  A file refused as 'unsupported' (progressive, ...) goes to fallback(bytes) -> uint8 BGR ndarray
    and becomes a host source; without a fallback, and for a corrupt file always, PPYoloHipError names the record."""
    if decoder is None:
        from .jpeg import JpegDecoder
        decoder = JpegDecoder()
    out, pend = [], []          # pend: (record to fill, its name for messages, bytes)

    def visit(rec, name):
        rec = dict(rec)
        im = rec.get('image')
        if im is None or isinstance(im, (bytes, bytearray, memoryview)):
            if im is None:
                if not rec.get('im_file'):
                    raise PPYoloHipError('%s has neither an image nor an im_file' % name)
                name = '%s (%s)' % (name, rec['im_file'])
                with open(rec['im_file'], 'rb') as fh:
                    im = fh.read()
            pend.append((rec, name, bytes(im)))
        if with_mixup and rec.get('mixup') is not None:
            rec['mixup'] = visit(rec['mixup'], name.split(' (')[0] + "['mixup']")
        return rec

    for i, rec in enumerate(records):
        out.append(visit(rec, 'record %d' % i))

    def done(rec, im):
        rec['image'] = im
        rec['h'], rec['w'] = int(im.shape[0]), int(im.shape[1])      # DecodeImage: set, or corrected from the decoded image

    refusal = getattr(decoder, 'refusal', None)
    good = []
    for rec, name, data in pend:
        r = refusal(data) if refusal is not None else None
        if r is None:
            good.append((rec, name, data))
            continue
        kind, reason = r
        if kind != 'unsupported' or fallback is None:
            raise PPYoloHipError('%s: %s JPEG: %s' % (name, kind, reason))
        im = fallback(data)
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise PPYoloHipError('%s: the fallback must return a uint8 BGR array [h, w, 3]' % name)
        done(rec, im)
    if good:
        try:
            ims = decoder.decode([g[2] for g in good])
        except PPYoloHipError as e:                 # 'item k: ...' of the decoder's list -> the record it came from
            m = re.match(r'item (\d+): (.*)', str(e), re.S)
            if m is None or int(m.group(1)) >= len(good):
                raise
            raise PPYoloHipError('%s: %s' % (good[int(m.group(1))][1], m.group(2))) from e
        if len(ims) != len(good):
            raise PPYoloHipError('the decoder returned %d images for %d files' % (len(ims), len(good)))
        for (rec, _, _), im in zip(good, ims):
            done(rec, im)
    return out


def _color_dtype(ops_):
    if not ops_:
        return U8
    return F64 if ops_[-1][0] == OP_HUE else F32


# ---------------------------------------------------------------------------------------------------------------------
# The device blob: descriptors (struct AugSample of csrc/augment.hip, 8-byte fields first), tables, source pixels,
# target element offsets / values, boxes.  Offsets are bytes from the start of the blob.  An EXTERNAL source (is_external)
# puts no pixel into the blob: its descriptor field holds its index in layout['sources'] and the ext flag is set.

DESC_I64 = 8            # src0, src1, xfirst, xw, yfirst, yw, ext0, ext1 (1: src is an index into the source table)
DESC_F64 = 9 + 4        # hue matrix t; f32(factor), f32(1 - factor) of mixup; two spare
DESC_I32 = 32
DESC_BYTES = 8 * DESC_I64 + 8 * DESC_F64 + 4 * DESC_I32


def _desc(r, to_rgb, off):
    i64 = np.zeros(DESC_I64, np.int64)
    f64 = np.zeros(DESC_F64, np.float64)
    i32 = np.zeros(DESC_I32, np.int32)
    i64[:] = [off['src0'], off['src1'], off['xfirst'], off['xw'], off['yfirst'], off['yw'], off['ext0'], off['ext1']]
    h0, w0 = (int(v) for v in r['image'].shape[:2])
    h1, w1 = ((int(v) for v in r['mix_image'].shape[:2]) if r['mix_image'] is not None else (0, 0))
    ops_ = r['ops']
    f32 = np.zeros(8, np.float32)
    codes = np.full(4, -1, np.int32)
    for k, (code, delta, t) in enumerate(ops_):
        codes[k] = code
        if code == OP_HUE:
            f64[:9] = t.reshape(-1)
        else:
            f32[2 * k] = np.float32(delta)
            f32[2 * k + 1] = np.float32(1.0 - delta)
    if r['factor'] is not None:
        f64[9], f64[10] = np.float32(r['factor']), np.float32(1.0 - r['factor'])
    eh, ew, ey, ex = r['expand'] if r['expand'] is not None else (0, 0, 0, 0)
    cy, cx, ch, cw = r['crop']
    rp = r['resize']
    i32[:] = [h0, w0, h1, w1, max(h0, h1), max(w0, w1), len(ops_), eh, ew, ey, ex,
              int(r['fill'][0]), int(r['fill'][1]), int(r['fill'][2]), cy, cx, ch, cw, int(r['flip']),
              r['color_dtype'], r['canvas_dtype'], rp['mode'], rp['fixpt'], rp['xw'].shape[1], rp['yw'].shape[1],
              rp['ix'], rp['iy'], int(bool(to_rgb)), codes[0], codes[1], codes[2], codes[3]]
    return i64.tobytes() + f64.tobytes() + i32.tobytes() + f32.tobytes()


DESC_BYTES += 32        # the eight float32 op constants (delta, 1 - delta) x 4


def pack_batch(recipes, to_rgb, toff, tval, gt_bbox, gt_class, gt_score):
    """-> (uint8 blob, layout dict of byte offsets).  Every part starts on a 16-byte boundary.  layout['sources']: the
    external sources in table order, the two of one sample next to each other (a tensor several samples use is listed once
    per use); empty for recipes whose images are all host arrays, whose blob is what it always was."""
    parts, pos = [], [0]

    def put(b):
        o = pos[0]
        parts.append(b)
        pos[0] += len(b)
        pad = (-pos[0]) % 16
        if pad:
            parts.append(b'\0' * pad)
            pos[0] += pad
        return o

    layout = dict(desc=put(b'\0' * (DESC_BYTES * len(recipes))))
    descs, sources = [], []

    def source(im):             # -> (src, ext)
        if is_external(im):
            sources.append(im)
            return len(sources) - 1, 1
        if isinstance(im, torch.Tensor):
            im = im.numpy()
        return put(np.ascontiguousarray(im).tobytes()), 0

    for r in recipes:
        off = {}
        off['src0'], off['ext0'] = source(r['image'])
        off['src1'], off['ext1'] = source(r['mix_image']) if r['mix_image'] is not None else (0, 0)
        rp = r['resize']
        off['xfirst'] = put(rp['xfirst'].astype(np.int32).tobytes())
        off['xw'] = put(rp['xw'].astype(np.float32).tobytes())
        off['yfirst'] = put(rp['yfirst'].astype(np.int32).tobytes())
        off['yw'] = put(rp['yw'].astype(np.float32).tobytes())
        descs.append(_desc(r, to_rgb, off))
    layout['sources'] = sources
    layout['toff'] = put(np.asarray(toff, np.int64).tobytes())
    layout['tval'] = put(np.asarray(tval, np.float32).tobytes())
    for k, a in (('gt_bbox', gt_bbox), ('gt_class', gt_class), ('gt_score', gt_score)):
        if a is not None:
            layout[k] = put(np.ascontiguousarray(a).tobytes())
    blob = np.frombuffer(b''.join(parts), np.uint8).copy()
    d = b''.join(descs)
    assert all(len(x) == DESC_BYTES for x in descs)
    blob[layout['desc']:layout['desc'] + len(d)] = np.frombuffer(d, np.uint8)
    return blob, layout
