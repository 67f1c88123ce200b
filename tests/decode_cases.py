"""Inputs of the YOLO decode kernels (csrc/decode_nms.hip: yolo_decode_body = "staged", yolo_decode_stream_kernel =
"streaming") beyond the one COCO layout, and the two oracle runs they are judged by  --  device-free TEST INFRASTRUCTURE
(tests/test_decode_cases.py checks the builders' own conditions on the CPU, tests/test_gpu_decode_edges.py runs the kernels).

A Case holds the head outputs (NCHW float32, one per level), anchors, strides, A, C, scale_x_y, iou_aware, factor, clip,
im_size [N, 2] (rows = (h, w)), thr (the float32 value, as a Python float) and `meta`.  `oracle(name, dtype)` is
oracle.ppyolo_oracle.iou_aware_score then yolo_box per level, levels concatenated as decode_all does: float32 = the reference's
arithmetic, float64 = every input cast to float64.  Two kinds of case:

  * LAYOUT cases: random logits N(0, 1.5) plus a bias on the IoU / objectness / class logits, picked from a fixed grid so that
    the share of (box, class) pairs above the threshold is nearest to one half (30 .. 70 %, `meta['share']`): eight head
    layouts (A, C, iou_aware), S in {1, 5, 9, 13} (81 cells = one 64-cell workgroup + 17 = five 16-cell groups + 1; 169 = two
    + 41), every value of scale_x_y / factor / clip / thr at least once and once on a (3, 80) layout, 1 .. 3 images, a
    two-level and a three-level case.  `all_pass` (bias +6) overflows the kernels' LDS lists.
  * EDGE cases at (3, 80), S = 9, N = 2: chosen logits in named (image, cell, anchor, class) slots -- the threshold ladder, the
    two clamps of the IoU-aware re-encoding, box extremes, the thresholds 0, -0.5 and 1.  `meta['slots']` names them.

Scores whose float64 value is below the smallest normal float32 have no float32 relative error (they underflow); `e32` and
the kernels' score error are taken over the others (`normal_scores`).
"""
import functools
import math

import numpy as np
import torch

from oracle import ppyolo_oracle as orc

RATIO_BOUND = 4.0            # kernel error <= RATIO_BOUND x the float32 oracle's own error (tests/test_gpu_loss_edges.py)
ERR_FLOOR = 1e-7             # one float32 rounding, the floor under the oracle's error
BAND_CAP = 1e-4              # at most this share of a case's pairs may sit in the threshold band
FLT_MIN = float(np.finfo(np.float32).tiny)
ANCHORS9 = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]
IM_SIZES = [(480., 640.), (375., 500.), (37., 1920.)]
STRIDE_OF = {1: 32, 5: 32, 9: 16, 13: 8}
BIAS_GRID = [0.5 * i for i in range(-16, 17)]


def f32(v):
    return float(np.float32(v))


class Case(object):
    def __init__(self, name, outs, anchors, strides, A, C, scale_x_y, iou_aware, factor, clip, im_size, thr, meta):
        self.name, self.outs, self.anchors, self.strides, self.A, self.C = name, outs, anchors, strides, A, C
        self.scale_x_y, self.iou_aware, self.factor, self.clip, self.im_size, self.thr, self.meta = \
            scale_x_y, bool(iou_aware), factor, bool(clip), im_size, f32(thr), meta

    @property
    def N(self):
        return self.outs[0].shape[0]

    @property
    def nch(self):
        return self.A * (5 + self.C) + (self.A if self.iou_aware else 0)

    @property
    def sizes(self):
        return [o.shape[2] for o in self.outs]

    @property
    def M(self):
        return sum(S * S * self.A for S in self.sizes)

    @property
    def pairs(self):
        return self.N * self.M * self.C

    def channel(self, a, j):
        """Channel of logit j (0 x, 1 y, 2 w, 3 h, 4 obj, 5 + c class c; -1 the IoU logit) of anchor a."""
        if j < 0:
            assert self.iou_aware
            return a
        return (self.A if self.iou_aware else 0) + a * (5 + self.C) + j

    def box(self, cell, a, level=0):
        """Row of (cell, anchor) of `level` in the concatenated boxes."""
        return sum(S * S * self.A for S in self.sizes[:level]) + cell * self.A + a


def _decode(case, dtype, clip=None):
    im = case.im_size.to(dtype)
    boxes, scores = [], []
    for o, anc, st in zip(case.outs, case.anchors, case.strides):
        o = o.to(dtype)
        if case.iou_aware:
            o = orc.iou_aware_score(o, case.A, case.C, case.factor)
        b, s = orc.yolo_box(o, np.asarray(anc, dtype=np.float32), st, case.C, case.scale_x_y, im,
                            case.clip if clip is None else clip)
        boxes.append(b)
        scores.append(s)
    return torch.cat(boxes, 1), torch.cat(scores, 1)


def _make(name, A, C, iou_aware, sizes, N, scale_x_y, factor, clip, thr, seed, bias=None, kind='layout'):
    g = torch.Generator().manual_seed(seed)
    nch = A * (5 + C) + (A if iou_aware else 0)
    raw = [torch.randn(N, nch, S, S, generator=g) * 1.5 for S in sizes]
    if len(sizes) == 1:
        anchors = [ANCHORS9[:A]]
    else:                                          # deepest level first, as the head orders them
        anchors = [ANCHORS9[6:9], ANCHORS9[3:6], ANCHORS9[0:3]][:len(sizes)]
    case = Case(name, raw, anchors, [STRIDE_OF[S] for S in sizes], A, C, scale_x_y, iou_aware, factor, clip,
                torch.tensor(IM_SIZES[:N]), thr, dict(kind=kind, seed=seed, slots={}))

    def biased(b):
        outs = []
        for o in raw:
            o = o.clone()
            for a in range(A):
                if iou_aware:
                    o[:, case.channel(a, -1)] += b
                o[:, case.channel(a, 4):case.channel(a, 5 + C)] += b          # objectness and the class logits
            outs.append(o)
        return outs

    def share(b):
        case.outs = biased(b)
        return (_decode(case, torch.float64)[1] > case.thr).double().mean().item()
    if bias is None:
        bias = min(BIAS_GRID, key=lambda b: (abs(share(b) - 0.5), b))
    case.meta['bias'] = bias
    case.meta['share'] = share(bias)
    return case


# name -> (A, C, iou_aware, sizes, N, scale_x_y, factor, clip, thr, seed)
LAYOUTS = {
    'l_3x80_ia_s9': (3, 80, True, (9,), 2, 1.05, 0.4, True, 0.01, 11),
    'l_3x80_plain_s13': (3, 80, False, (13,), 3, 1.0, 0.4, False, 0.3, 12),
    'l_3x80_ia_s5_f1': (3, 80, True, (5,), 1, 1.2, 1.0, False, 0.3, 13),
    'l_3x80_ia_s1_f0': (3, 80, True, (1,), 2, 1.0, 0.0, True, 0.01, 14),
    'l_3x1_ia_s9': (3, 1, True, (9,), 3, 1.2, 0.4, False, 0.01, 15),
    'l_1x80_plain_s13': (1, 80, False, (13,), 2, 1.05, 0.4, True, 0.3, 16),
    'l_2x20_plain_s9': (2, 20, False, (9,), 1, 1.0, 0.4, True, 0.01, 17),
    'l_4x7_ia_s5': (4, 7, True, (5,), 3, 1.05, 1.0, False, 0.3, 18),
    'l_8x3_ia_s13': (8, 3, True, (13,), 2, 1.2, 0.0, True, 0.01, 19),
    'l_3x85_plain_s9': (3, 85, False, (9,), 2, 1.05, 0.4, False, 0.3, 20),          # nch = 270, the largest accepted
    'l_3x80_ia_two_levels': (3, 80, True, (5, 9), 2, 1.05, 0.4, True, 0.01, 21),
    'l_3x80_plain_three_levels': (3, 80, False, (5, 9, 13), 3, 1.2, 0.4, True, 0.3, 22),
}
NMS_CASES = ['l_3x1_ia_s9', 'l_2x20_plain_s9']
ALL_PASS = 'all_pass'


def _all_pass():
    return _make(ALL_PASS, 3, 80, True, (9,), 2, 1.05, 0.4, True, 0.01, 23, bias=6.0, kind='all_pass')


# ---------------------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _edge(name, iou_aware, thr=0.01, scale_x_y=1.05, clip=True, bias=-2.0, seed=31):
    return _make(name, 3, 80, iou_aware, (9,), 2, scale_x_y, 0.4, clip, thr, seed, bias=bias, kind='edge')


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def conf_scalar(x, iou_logit, factor, iou_aware):
    """Float64 confidence of an objectness logit x (oracle.iou_aware_score + sigmoid, one element)."""
    if not iou_aware:
        return _sig(x)
    new = _sig(x) ** (1.0 - factor) * _sig(iou_logit) ** factor
    new = min(max(new, 1e-7), 1e7)
    new = min(max(1.0 / new - 1.0, 1e-7), 1e7)
    return 1.0 / (1.0 + new)


def conf_of(case, dtype):
    """Confidence [N, M] of every (cell, anchor) as the oracle computes it in `dtype` (level 0 only)."""
    o = case.outs[0].to(dtype)
    if case.iou_aware:
        o = orc.iou_aware_score(o, case.A, case.C, case.factor)
    N, _, S, _ = o.shape
    o = o.permute(0, 2, 3, 1).reshape(N, S * S, case.A, 5 + case.C)
    return torch.sigmoid(o[..., 4]).reshape(N, S * S * case.A)


LADDER_LEN = 200
LADDER_D = [0.0] + [s * d for d in (1e-6, 1e-4, 1e-3, 0.02, 0.03, 0.1, 0.25) for s in (1.0, -1.0)]
LADDER_FIXED = [80.0, -80.0, float('inf'), float('-inf'), float('nan')]
LADDER_IOU_LOGIT = 30.0
LADDER_DEAD_CENTRE = 20.0            # class-logit centre of a ladder step with conf64 <= thr (thr / conf has no logit)


def ladder(iou_aware):
    """Objectness logits: LADDER_LEN consecutive float32 values centred on the logit whose float64 confidence is thr (IoU
    logit 30 when IoU-aware, so that the confidence follows the objectness alone) -- pairs 0 .. 199 of image 0 in (cell,
    anchor) order.  Classes 0 .. 19 of each: logit(thr / conf64) + d for d in LADDER_D, then +-80, +-inf, NaN."""
    c = _edge('ladder_%s' % ('ia' if iou_aware else 'plain'), iou_aware, seed=32)
    lo, hi = -30.0, 30.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if conf_scalar(mid, LADDER_IOU_LOGIT, c.factor, iou_aware) < c.thr:
            lo = mid
        else:
            hi = mid
    centre = np.array([hi], dtype=np.float32)
    steps = (centre.view(np.int32) + np.arange(-LADDER_LEN // 2, LADDER_LEN // 2, dtype=np.int32)).view(np.float32)
    S, o = c.sizes[0], c.outs[0]
    for q in range(LADDER_LEN):
        cell, a = divmod(q, c.A)
        h, w = divmod(cell, S)
        o[0, c.channel(a, 4), h, w] = float(steps[q])
        if iou_aware:
            o[0, c.channel(a, -1), h, w] = LADDER_IOU_LOGIT
    conf64 = conf_of(c, torch.float64)[0]
    slots = []
    for q in range(LADDER_LEN):
        cell, a = divmod(q, c.A)
        h, w = divmod(cell, S)
        tq = c.thr / conf64[q].item()
        centre_q = math.log(tq / (1.0 - tq)) if tq < 1.0 else LADDER_DEAD_CENTRE
        for k, v in enumerate([centre_q + d for d in LADDER_D] + LADDER_FIXED):
            o[0, c.channel(a, 5 + k), h, w] = v
            slots.append((0, c.box(cell, a), k))
    c.meta['slots']['ladder'] = slots
    c.meta['ladder_conf64'] = conf64[:LADDER_LEN].clone()
    return c


CLAMP_FIRST = [math.log(1e-7 / (1.0 - 1e-7)) + d for d in (-1.0, -0.1, -0.002, 0.002, 0.1, 1.0)]      # sigmoid = 1e-7 (1 + ~d)
CLAMP_SECOND = [14.0, 15.0, 15.8, 17.0, 20.0, 30.0]        # 1 / sigmoid - 1 = exp(-x): the kink 1e-7 is at x = 16.118


def iou_branches(case, dtype):
    """The two clamps of the IoU-aware re-encoding as `dtype` takes them: (new < 1e-7, 1 / new - 1 < 1e-7), each [N, M]."""
    o = case.outs[0].to(dtype)
    N, _, S, _ = o.shape
    A, per = case.A, 5 + case.C
    first, second = [], []
    for a in range(A):
        ioup, obj = torch.sigmoid(o[:, a]), torch.sigmoid(o[:, A + a * per + 4])
        new = torch.pow(obj, 1 - case.factor) * torch.pow(ioup, case.factor)
        first.append(new < 1e-7)
        second.append(1.0 / torch.clamp(new, 1e-7, 1e7) - 1.0 < 1e-7)
    shape = lambda parts: torch.stack(parts, -1).reshape(N, S * S * A)
    return shape(first), shape(second)


def iou_clamps():
    """(objectness, IoU) logit pairs, both at x: sigmoid(x) around 1e-7 (first clamp) and around 1 - 1e-7 (second clamp: the
    re-encoded logit saturates at -log(1e-7)), at least 1e-3 relative away from each kink."""
    c = _edge('iou_clamps', True, seed=33)
    S, o = c.sizes[0], c.outs[0]
    slots = []
    for n in range(c.N):
        for q, x in enumerate(CLAMP_FIRST + CLAMP_SECOND):
            cell, a = 7 * q + n, q % c.A
            h, w = divmod(cell, S)
            o[n, c.channel(a, 4), h, w] = x
            o[n, c.channel(a, -1), h, w] = x
            slots.append((n, c.box(cell, a), x))
    c.meta['slots']['clamp'] = slots
    return c


def box_extremes(iou_aware, clip):
    """tw / th at -100, 80 and 100 (float32 exp overflows at 88.7: with clip the reference's x0 * 0 then gives NaN), tx / ty
    at +-80, boxes wholly outside the image on each side (scale_x_y = 1.2 lets a centre leave the grid), a NaN cell, a NaN in the objectness / IoU logit alone."""
    c = _edge('box_%s_%s' % ('ia' if iou_aware else 'plain', 'clip' if clip else 'noclip'), iou_aware, scale_x_y=1.2, clip=clip, seed=34)
    S, o = c.sizes[0], c.outs[0]
    L = S - 1
    # (h, w, anchor) -> {logit index: value}
    table = {
        'tiny': ((4, 4, 0), {2: -100.0, 3: -100.0}),
        'huge': ((4, 5, 1), {2: 80.0, 3: 80.0}),
        'overflow': ((4, 6, 2), {2: 100.0, 3: 100.0}),
        'overflow_w': ((3, 3, 0), {2: 100.0}),
        'xy_hi_lo': ((2, 2, 1), {0: 80.0, 1: -80.0}),
        'xy_lo_hi': ((2, 3, 2), {0: -80.0, 1: 80.0}),
        'out_left': ((4, 0, 0), {0: -80.0, 2: -100.0, 3: -100.0}),
        'out_right': ((4, L, 0), {0: 80.0, 2: -100.0, 3: -100.0}),
        'out_top': ((0, 4, 1), {1: -80.0, 2: -100.0, 3: -100.0}),
        'out_bottom': ((L, 4, 1), {1: 80.0, 2: -100.0, 3: -100.0}),
    }
    for n in range(c.N):
        for key, ((h, w, a), vals) in table.items():
            for j, v in vals.items():
                o[n, c.channel(a, j), h, w] = v
            c.meta['slots'].setdefault(key, []).append((n, c.box(h * S + w, a)))
    o[1, :, L, L] = float('nan')
    c.meta['slots']['nan_cell'] = [(1, c.box(L * S + L, a)) for a in range(c.A)]
    # a NaN in the objectness (or, IoU-aware, in the IoU logit) alone: torch.clamp keeps it, every score of the pair is NaN
    # while its box and its class logits are finite
    lone = [((6, 6, 2), 4)] + ([((6, 7, 0), -1)] if iou_aware else [])
    for (h, w, a), j in lone:
        o[0, c.channel(a, j), h, w] = float('nan')
        c.meta['slots'].setdefault('nan_conf', []).append((0, c.box(h * S + w, a)))
    return c


def thresholds(thr, iou_aware):
    """thr = 0, -0.5 or 1 (no band: the reference's float32 `score > thr` decides).  One pair of image 0 has class logits -inf
    (score +0), -200 (score underflows to +0), +inf and NaN; one pair has objectness 80 and a class logit of 80."""
    c = _edge('thr_%s_%s' % ({0.0: 'zero', -0.5: 'negative', 1.0: 'one'}[thr], 'ia' if iou_aware else 'plain'), iou_aware,
              thr=thr, bias=0.0, seed=35)
    S, o = c.sizes[0], c.outs[0]
    (h, w), a = divmod(10, S), 1
    for k, v in ((3, float('-inf')), (4, -200.0), (5, float('inf')), (6, float('nan'))):
        o[0, c.channel(a, 5 + k), h, w] = v
    b = c.box(10, a)
    c.meta['slots'].update(neg_inf=[(0, b, 3)], underflow=[(0, b, 4)], pos_inf=[(0, b, 5)], nan=[(0, b, 6)])
    (h, w), a = divmod(11, S), 0
    o[0, c.channel(a, 4), h, w] = 80.0
    o[0, c.channel(a, 5), h, w] = 80.0
    c.meta['slots']['saturated'] = [(0, c.box(11, a), 0)]
    return c


EDGES = {}
for _ia in (True, False):
    _t = 'ia' if _ia else 'plain'
    EDGES['ladder_' + _t] = functools.partial(ladder, _ia)
    for _clip in (True, False):
        EDGES['box_%s_%s' % (_t, 'clip' if _clip else 'noclip')] = functools.partial(box_extremes, _ia, _clip)
    for _thr, _nm in ((0.0, 'zero'), (-0.5, 'negative'), (1.0, 'one')):
        EDGES['thr_%s_%s' % (_nm, _t)] = functools.partial(thresholds, _thr, _ia)
EDGES['iou_clamps'] = iou_clamps
NO_BAND = sorted(n for n in EDGES if n.startswith('thr_'))            # judged by the float32 rule alone


def names():
    return sorted(LAYOUTS) + [ALL_PASS] + sorted(EDGES)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases and their oracle runs (computed once per case and precision; the results are shared -- do not modify them)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def get(name):
    if name in LAYOUTS:
        return _make(name, *LAYOUTS[name])
    if name == ALL_PASS:
        return _all_pass()
    return EDGES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float32):
    """-> (boxes [N, M, 4], scores [N, M, C]) of case `name` in `dtype`."""
    return _decode(get(name), dtype)


@functools.lru_cache(maxsize=None)
def unclipped(name, dtype):
    return _decode(get(name), dtype, clip=False)[0]


def normal_scores(name):
    """Pairs whose float64 score is finite and a normal float32: the ones a relative error is taken over."""
    s64 = oracle(name, torch.float64)[1]
    return torch.isfinite(s64) & (s64 >= FLT_MIN)


def rel_score_error(scores, name):
    """Largest |scores - score64| / score64 over normal_scores (scores: float32 [N, M, C])."""
    s64, ok = oracle(name, torch.float64)[1], normal_scores(name)
    ok = ok & torch.isfinite(scores)
    if not ok.any():
        return 0.0
    return ((scores.double()[ok] - s64[ok]).abs() / s64[ok]).max().item()


def rel_box_error(boxes, name):
    """Largest |boxes - box64| / max(1, |box64|) over the entries finite in `boxes`, the float32 oracle and float64."""
    b64, b32 = oracle(name, torch.float64)[0], oracle(name, torch.float32)[0]
    ok = torch.isfinite(b64) & torch.isfinite(b32) & torch.isfinite(boxes)
    if not ok.any():
        return 0.0
    return ((boxes.double()[ok] - b64[ok]).abs() / b64[ok].abs().clamp(min=1.0)).max().item()


@functools.lru_cache(maxsize=None)
def e32(name):
    """Largest relative error of the float32 oracle's scores against float64."""
    return rel_score_error(oracle(name, torch.float32)[1], name)


@functools.lru_cache(maxsize=None)
def band(name):
    """Pairs [N, M, C] whose float64 score is so near the threshold that either decision is right:
    |score64 / thr - 1| <= RATIO_BOUND * e32.  Empty for the NO_BAND cases."""
    c, s64 = get(name), oracle(name, torch.float64)[1]
    if name in NO_BAND:
        return torch.zeros_like(s64, dtype=torch.bool)
    return (s64 / c.thr - 1.0).abs() <= RATIO_BOUND * e32(name)


def slot_mask(name, key):
    """Bool [N, M, C] of the (image, box, class) slots `key` of an edge case."""
    c = get(name)
    m = torch.zeros(c.N, c.M, c.C, dtype=torch.bool)
    for n, b, k in c.meta['slots'][key]:
        m[n, b, k] = True
    return m


def score_to_key(s):
    """csrc/nms_select.h: the unsigned order key of a float32 score (numpy float32 array -> uint32 as int64)."""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, (~b) & 0xffffffff, b ^ 0x80000000)
