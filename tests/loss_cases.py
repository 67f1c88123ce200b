"""Inputs of ppy_yolov3_loss_f32 (csrc/yolo_loss.hip) at its kinks and edges, and the two oracle runs they are judged by  --
device-free TEST INFRASTRUCTURE (tests/test_loss_cases.py checks the builders' own conditions on the CPU,
tests/test_gpu_loss_edges.py runs the kernel on them).

Every builder returns a Case: (out NCHW float32, target [N, an, 6+C, S, S], gt_box [N, G, 4], cfg, meta).  Two kinds:

  * MARGIN cases (`geometry`): random logits at the shapes where the kernel's index arithmetic changes (partial / exact /
    straddled workgroups, class splits with empty and ragged parts, 1 .. 4 anchors, a row wider than the workgroup), every
    kink of the loss kept at a distance (`margins`) so that float32 and float64 agree on every branch and the float64
    oracle is the exact answer.
  * TIE cases (`SEMANTICS`): inputs that sit exactly ON a kink (|.| at 0, min / max ties, clamp at 0, a NaN in the ignore
    mask's maximum, a saturated sigmoid).  Float64 decides those differently (exp(-120) is not 0 there), so they are judged by
    the float32 oracle = the reference's arithmetic and torch autograd's tie rules.  `meta['ties']` lists, per case, the
    gradient elements the tie decides: the loss term to isolate, the element, the value the intended share gives and the
    `unit` = how far the element moves when the share is off by 0.5 (or a gate by 1).
"""
import copy
import functools
import math

import torch

from config import PPYOLO_2x_Config
from oracle import ppyolo_oracle as orc
from oracle import train_oracle as trn

LOSS_NAMES = ['loss_xy', 'loss_wh', 'loss_obj', 'loss_cls', 'loss_iou', 'loss_iou_aware']      # order of the kernel's loss6
CELLS_PER_WORKGROUP = 64                                                                       # LOSS_CELLS of csrc/yolo_loss.hip
NUM_GT = 12


class Case(object):
    def __init__(self, name, out, target, gt, cfg, meta):
        self.name, self.out, self.target, self.gt, self.cfg, self.meta = name, out, target, gt, cfg, meta

    def __iter__(self):
        return iter((self.out, self.target, self.gt, self.cfg, self.meta))


def channel(meta, a, j):
    """Channel of logit j (0 x, 1 y, 2 w, 3 h, 4 obj, 5 + c class c) of anchor a in the head output."""
    return (meta['an'] if meta['iou_aware'] else 0) + a * (5 + meta['C']) + j


def slice_of(meta, ch):
    """Name of the split_grad tensor that channel `ch` of the head output belongs to."""
    if meta['iou_aware']:
        if ch < meta['an']:
            return 'ioup'
        ch -= meta['an']
    j = ch % (5 + meta['C'])
    return ['x', 'y', 'w', 'h', 'obj'][j] if j < 5 else 'cls'


def split_grad(d, meta):
    """d loss / d head output [N, nch, S, S] -> the tensors the loss splits it into (losses.py:243-270)."""
    an, C = meta['an'], meta['C']
    parts = {}
    if meta['iou_aware']:
        parts['ioup'], d = d[:, :an], d[:, an:]
    o = d.reshape(d.shape[0], an, 5 + C, d.shape[2], d.shape[3])
    for j, k in enumerate(['x', 'y', 'w', 'h', 'obj']):
        parts[k] = o[:, :, j]
    parts['cls'] = o[:, :, 5:]
    return parts


def _positions(N, S, an):
    """Positives (n, a, cell, score): the first and the last cell of every workgroup, both sides of every workgroup boundary
    (64k-1 | 64k: one grid row, or two) on ONE anchor, and cells 0 and S-1 of grid row 0 on one anchor -- rows with two
    positives of an anchor make the IoU-aware broadcast T = sum_w tobj differ from tobj.  gt_score < 1 on the second of a pair."""
    cells = S * S
    pos = {}
    for n in range(N):
        a0 = n % an
        pairs = [(0, S - 1)] if S > 1 else []
        pairs += [(CELLS_PER_WORKGROUP * k - 1, CELLS_PER_WORKGROUP * k) for k in range(1, (cells - 1) // CELLS_PER_WORKGROUP + 1)]
        for i, (c0, c1) in enumerate(pairs):
            pos.setdefault((n, (a0 + i) % an, c0), 1.0)
            pos.setdefault((n, (a0 + i) % an, c1), 0.6)
        for i, c in enumerate(sorted({0, min(CELLS_PER_WORKGROUP - 1, cells - 1), cells - 1, cells // 2})):
            pos.setdefault((n, (a0 + 1 + i) % an, c), 0.8 if (i + n) % 2 == 1 else 1.0)
    return [(n, a, c, s) for (n, a, c), s in sorted(pos.items())]


def _base(name, N, S, an, C, iou_aware, seed, scale_x_y=1.05, loss_square=True, ignore_thresh=0.7, mask=None, ignored=True):
    cfg = PPYOLO_2x_Config()
    mask = list(mask if mask is not None else {1: [4], 2: [3, 4], 3: [3, 4, 5], 4: [2, 3, 4, 5]}[an])
    cfg.head = dict(cfg.head, num_classes=C, anchor_masks=[mask], downsample=[32], iou_aware=iou_aware)
    cfg.yolo_loss = dict(cfg.yolo_loss, scale_x_y=scale_x_y, ignore_thresh=ignore_thresh)
    cfg.iou_loss = dict(cfg.iou_loss, loss_square=loss_square)
    anchors = [list(cfg.head['anchors'][m]) for m in mask]
    meta = dict(N=N, S=S, an=an, C=C, iou_aware=bool(iou_aware), anchors=anchors, downsample=32, scale_x_y=scale_x_y,
                ignore_thresh=ignore_thresh, loss_square=loss_square, w_iou=cfg.iou_loss['loss_weight'],
                w_iou_aware=cfg.iou_aware_loss['loss_weight'] if iou_aware else 0.0, seed=seed, ties=[])
    g = torch.Generator().manual_seed(seed)
    nch = an * (5 + C) + (an if iou_aware else 0)
    out = torch.randn(N, nch, S, S, generator=g) * 0.7
    tgt = torch.zeros(N, an, 6 + C, S, S)
    gt = torch.zeros(N, NUM_GT, 4)
    positives = []
    rows = [0] * N
    for n, a, cell, score in _positions(N, S, an):
        h, w = divmod(cell, S)
        tgt[n, a, 0:2, h, w] = 0.1 + 0.8 * torch.rand(2, generator=g)
        tgt[n, a, 2:4, h, w] = torch.randn(2, generator=g) * 0.3
        tgt[n, a, 4, h, w] = 1.0 + torch.rand(1, generator=g).item()
        tgt[n, a, 5, h, w] = score
        tgt[n, a, 6 + int(torch.randint(0, C, (1,), generator=g)), h, w] = 1.0
        positives.append((n, a, h, w))
        if rows[n] < NUM_GT - 2:                     # the ground-truth box this target was made from
            t = tgt[n, a, :, h, w]
            gt[n, rows[n]] = torch.tensor([(w + t[0].item()) / S, (h + t[1].item()) / S,
                                           math.exp(t[2].item()) * anchors[a][0] / (S * 32), math.exp(t[3].item()) * anchors[a][1] / (S * 32)])
            rows[n] += 1
    meta['positives'] = positives
    meta['ignored'] = []
    if ignored:
        # a ground-truth box of another level that coincides with a NEGATIVE cell's prediction: best IoU ~ 1, the cell is ignored
        taken = set(positives)
        for n in range(N):
            cand = [(n, a, h, w) for a in range(an) for h in range(S) for w in range(S) if (n, a, h, w) not in taken]
            if not cand:
                continue
            _, a, h, w = cand[(len(cand) * 2) // 3]
            o = out[n, :, h, w].double()
            sx, sy = torch.sigmoid(o[channel(meta, a, 0)]).item(), torch.sigmoid(o[channel(meta, a, 1)]).item()
            gt[n, rows[n]] = torch.tensor([(scale_x_y * sx - 0.5 * (scale_x_y - 1.0) + w) / S, (scale_x_y * sy - 0.5 * (scale_x_y - 1.0) + h) / S,
                                           math.exp(o[channel(meta, a, 2)].item()) * anchors[a][0] / (S * 32),
                                           math.exp(o[channel(meta, a, 3)].item()) * anchors[a][1] / (S * 32)])
            rows[n] += 1
            meta['ignored'].append((n, a, h, w))
    return Case(name, out, tgt, gt, cfg, meta)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the geometry matrix: margin cases.  (N, S, an, C) -> seed per iou_aware (picked on the CPU so that `margins` holds with
# every cell counted; tests/test_loss_cases.py asserts it)
# ---------------------------------------------------------------------------------------------------------------------------------
GEOMETRY = [(2, 1, 3, 80), (2, 7, 3, 80), (1, 8, 2, 20), (3, 9, 3, 11), (2, 13, 4, 9), (2, 9, 1, 1), (2, 9, 1, 3), (1, 9, 1, 300),
            (2, 13, 3, 91)]
GEOMETRY_SEEDS = {}


def geometry_name(shape, iou_aware):
    return 'geo_%dx%dx%dx%d_%s' % (shape + ('ia' if iou_aware else 'plain',))


def geometry(shape, iou_aware, seed=None):
    name = geometry_name(shape, iou_aware)
    return _base(name, *shape, iou_aware=iou_aware, seed=GEOMETRY_SEEDS.get(name, 1) if seed is None else seed)


def _decoded(case, dtype=torch.float64):
    out, tgt, gt, cfg, m = case
    out, tgt = out.to(dtype), tgt.to(dtype)
    an, C = m['an'], m['C']
    body = out[:, an:] if m['iou_aware'] else out
    x, y, w, h, obj, _ = trn.split_output(body, an, C)
    tx, ty, tw, th, tscale, tobj, _ = trn.split_target(tgt)
    return body, (x, y, w, h, obj), (tx, ty, tw, th, tscale, tobj)


def margins(case):
    """Float64 distances of a case from every kink of the loss, minimum over ALL cells concerned (none filtered), and the counts
    that show the case exercises what it is meant to."""
    out, tgt, gt, cfg, m = case
    body, (x, y, w, h, obj), (tx, ty, tw, th, tscale, tobj) = _decoded(case)
    s = m['scale_x_y']
    anchors = [v for a in m['anchors'] for v in a]
    ts = tscale * tobj
    pos = ts > 0
    res = {}
    boxes = trn.train_boxes(body, torch.tensor(m['anchors'], dtype=torch.float64).numpy(), m['downsample'], m['C'], s)
    best = []
    for pred, g in zip(boxes, gt.double()):
        gg = torch.cat([g[:, 0:1] - g[:, 2:3] / 2., g[:, 1:2] - g[:, 3:4] / 2., g[:, 0:1] + g[:, 2:3] / 2., g[:, 1:2] + g[:, 3:4] / 2.], 1)
        best.append(orc.pairwise_iou(pred, gg).max(-1)[0])
    best = torch.stack(best).reshape(tobj.shape)
    res['n_nan'] = int(torch.isnan(best).sum())
    res['ignore'] = (best[~torch.isnan(best)] - m['ignore_thresh']).abs().min().item()
    res['n_ignored_negatives'] = int(((best > m['ignore_thresh']) & ~(tobj > 0)).sum())
    res['n_counted_negatives'] = int(((best <= m['ignore_thresh']) & ~(tobj > 0)).sum())
    inf = torch.tensor(float('inf'), dtype=torch.float64)
    if abs(s - 1.0) > 1e-10:
        px, py = s * torch.sigmoid(x) - 0.5 * (s - 1.0), s * torch.sigmoid(y) - 0.5 * (s - 1.0)
        res['xy'] = torch.where(pos, torch.min((px - tx).abs(), (py - ty).abs()), inf).min().item()
    res['wh'] = torch.where(pos, torch.min((w - tw).abs(), (h - th).abs()), inf).min().item()
    T = tobj.sum(-1, keepdim=True).expand_as(tobj)
    recv = pos | ((T != 0) if m['iou_aware'] else torch.zeros_like(pos))
    x1, y1, x2r, y2r = trn.bbox_transform(x, y, w, h, anchors, m['downsample'], False, s)
    x1g, y1g, x2g, y2g = trn.bbox_transform(tx, ty, tw, th, anchors, m['downsample'], True, s)
    x2, y2 = torch.max(x1, x2r), torch.max(y1, y2r)
    ops = [x2r - x1, y2r - y1, x2 - x2g, y2 - y2g, x1 - x1g, y1 - y1g,
           torch.min(x2, x2g) - torch.max(x1, x1g), torch.min(y2, y2g) - torch.max(y1, y1g)]
    res['iou'] = min(torch.where(recv, o.abs(), inf).min().item() for o in ops)
    res['n_positives'] = int(pos.sum())
    res['n_iou_aware_only'] = int((recv & ~pos).sum())                   # tobj = 0 in a row with T != 0
    res['n_broadcast_rows'] = int(((tobj > 0).sum(-1) >= 2).sum())       # (image, anchor, grid row) with two positives
    res['n_soft_scores'] = int(((tobj > 0) & (tobj < 1)).sum())
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the semantics cases: tie cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _ts(case, n, a, h, w):
    return (case.target[n, a, 4, h, w] * case.target[n, a, 5, h, w]).item()


def wh_tie():
    """lw == tw and lh == th bit for bit on every positive: d |lw - tw| = sign(0) = 0, the w / h gradient is the IoU part alone."""
    c = _base('wh_tie', 2, 9, 3, 11, True, seed=101)
    m = c.meta
    for n, a, h, w in m['positives']:
        c.out[n, channel(m, a, 2), h, w] = c.target[n, a, 2, h, w]
        c.out[n, channel(m, a, 3), h, w] = c.target[n, a, 3, h, w]
        for j in (2, 3):
            m['ties'].append(dict(term='loss_wh', idx=(n, channel(m, a, j), h, w), want=0.0, unit=0.5 * _ts(c, n, a, h, w) / m['N'], exact=True))
    return c


def xy_tie():
    """x = y = 0 and tx = ty = the float32 value of scale_x_y * 0.5 - 0.5 * (scale_x_y - 1) as the reference computes it (the
    product with 0.5 is exact, so a contracted multiply-subtract gives the same bits): d |px - tx| = sign(0) = 0."""
    c = _base('xy_tie', 2, 9, 3, 11, True, seed=102)
    m = c.meta
    s = m['scale_x_y']
    t0 = (s * torch.sigmoid(torch.zeros(1)) - 0.5 * (s - 1.0)).item()
    for n, a, h, w in m['positives']:
        for j in (0, 1):
            c.out[n, channel(m, a, j), h, w] = 0.0
            c.target[n, a, j, h, w] = t0
            m['ties'].append(dict(term='loss_xy', idx=(n, channel(m, a, j), h, w), want=0.0, unit=0.5 * _ts(c, n, a, h, w) * s * 0.25 / m['N'], exact=True))
    return c


def identical_boxes(square):
    """scale_x_y = 1, x = y = 0, tx = ty = 0.5, lw = tw, lh = th: the decoded box IS the target box, all four min / max of the
    intersection tie.  With share s for the prediction's operand, d k / d lw = (2 s - 1) (+ O(1e-10 / area)): torch's 0.5 gives 0,
    a share of 1 gives d loss_iou / d k itself."""
    c = _base('identical_%s' % ('square' if square else 'linear'), 2, 9, 3, 11, False, seed=103, scale_x_y=1.0, loss_square=square)
    m = c.meta
    # loss_iou = (1 - k^2) * weight * ts with k = 1 - O(float32 rounding): the float32 oracle's value is exactly 0 by cancellation,
    # so the term's error is judged relative to its summands' scale weight * ts (the value at k = 0)
    m['loss_scale'] = {'loss_iou': sum(m['w_iou'] * _ts(c, *p) for p in m['positives']) / m['N']}
    for n, a, h, w in m['positives']:
        c.out[n, channel(m, a, 0), h, w] = 0.0
        c.out[n, channel(m, a, 1), h, w] = 0.0
        c.target[n, a, 0:2, h, w] = 0.5
        c.out[n, channel(m, a, 2), h, w] = c.target[n, a, 2, h, w]
        c.out[n, channel(m, a, 3), h, w] = c.target[n, a, 3, h, w]
        dk = (2.0 if square else 1.0) * m['w_iou'] * _ts(c, n, a, h, w)          # |d loss_iou / d k| at k = 1
        for j in (2, 3):
            m['ties'].append(dict(term='loss_iou', idx=(n, channel(m, a, j), h, w), want=0.0, unit=0.5 * dk / m['N'], exact=False))
    return c


DEGENERATE_LOGIT = -120.0          # exp() is 0 in float32: x1 == x2, y1 == y2, a box of area 0


def degenerate():
    """Predictions of zero size (lw = lh = -120), loss_square = False so that d loss / d k != 0 where k = 0.  On positives the
    max(x1, x2) tie and the clamp at exactly 0 are reached.  On NEGATIVE cells the ignore-mask IoU with a zero-padded gt row is
    0 / 0: torch.max propagates the NaN, `NaN <= ignore_thresh` is False, the cell contributes no negative objectness term --
    d / d obj is exactly 0 where a maximum that skipped the NaN would give sigmoid(obj) / N.  The NaN comes last in the row of
    image 0 (real boxes first) and first in image 1 (the gt rows reversed)."""
    c = _base('degenerate', 2, 9, 3, 11, True, seed=104, loss_square=False, ignored=False)
    m = c.meta
    for i, (n, a, h, w) in enumerate(m['positives']):
        if i % 2 == 0:
            c.out[n, channel(m, a, 2), h, w] = DEGENERATE_LOGIT
            c.out[n, channel(m, a, 3), h, w] = DEGENERATE_LOGIT
    c.gt[1] = c.gt[1].flip(0).clone()
    taken = set(m['positives'])
    m['nan_cells'] = []
    for n in range(m['N']):
        free = [(n, a, h, w) for a in range(m['an']) for h in range(m['S']) for w in range(m['S']) if (n, a, h, w) not in taken]
        for k in (1, len(free) // 2, len(free) - 2):
            _, a, h, w = free[k]
            c.out[n, channel(m, a, 2), h, w] = DEGENERATE_LOGIT
            c.out[n, channel(m, a, 3), h, w] = DEGENERATE_LOGIT
            c.out[n, channel(m, a, 4), h, w] = 2.0
            m['nan_cells'].append((n, a, h, w))
            m['ties'].append(dict(term='loss_obj', idx=(n, channel(m, a, 4), h, w), want=0.0, unit=torch.sigmoid(torch.tensor(2.0)).item() / m['N'], exact=True))
    return c


def disjoint():
    """Smallest anchors, tw = th = -3, loss_square = False.  Even positives: the prediction in the far corner of the cell --
    both extents of the intersection are negative.  Odd positives: disjoint along x only (ih > 0): there a clamp that passed
    the gradient would give d loss_iou / d lw = d loss / d k * ih * pw / union; torch.clamp gives exactly 0."""
    c = _base('disjoint', 2, 9, 3, 11, False, seed=105, loss_square=False, mask=[0, 1, 2])
    m = c.meta
    S = m['S']
    for i, (n, a, h, w) in enumerate(m['positives']):
        c.target[n, a, 0, h, w] = 0.05
        c.out[n, channel(m, a, 0), h, w] = 6.0
        c.target[n, a, 2:4, h, w] = -3.0
        c.out[n, channel(m, a, 2), h, w] = -3.2
        if i % 2 == 0:
            c.target[n, a, 1, h, w] = 0.05
            c.out[n, channel(m, a, 1), h, w] = 6.0
            c.out[n, channel(m, a, 3), h, w] = -3.2
        else:
            c.target[n, a, 1, h, w] = 0.5
            c.out[n, channel(m, a, 1), h, w] = 0.004
            c.out[n, channel(m, a, 3), h, w] = -2.9
            den = S * m['downsample']
            pw, pwg = math.exp(-3.2) * m['anchors'][a][0] / den, math.exp(-3.0) * m['anchors'][a][0] / den
            ph, phg = math.exp(-2.9) * m['anchors'][a][1] / den, math.exp(-3.0) * m['anchors'][a][1] / den
            py = m['scale_x_y'] / (1 + math.exp(-0.004)) - 0.5 * (m['scale_x_y'] - 1)
            ih = min(py / S + ph / 2, 0.5 / S + phg / 2) - max(py / S - ph / 2, 0.5 / S - phg / 2)
            assert ih > 0
            unit = m['w_iou'] * _ts(c, n, a, h, w) * ih * pw / (pw * ph + pwg * phg + 1e-10) / m['N']
            m['ties'].append(dict(term='loss_iou', idx=(n, channel(m, a, 2), h, w), want=0.0, unit=unit, exact=True))
    return c


SATURATED = [90.0, -90.0, 40.0, -40.0]         # sigmoid is exactly 1 / 0 in float32 at +-90; log(0 + 1e-9) is reached


def saturation(scale_x_y):
    """obj, x, y, ioup and class logits at +-90 and +-40, on positives and negatives: everything stays finite (the `+ 1e-9` inside
    the logarithms; 0 * 1e9 in the sigmoid's backward), with the gradients of the float32 oracle."""
    c = _base('saturation_%s' % ('grid' if scale_x_y != 1.0 else 'plain'), 2, 9, 3, 11, True, seed=106, scale_x_y=scale_x_y, ignored=False)
    m = c.meta
    S, k = m['S'], 0
    for i, (n, a, h, w) in enumerate(m['positives']):
        hot = int(c.target[n, a, 6:, h, w].argmax())
        for ch in (channel(m, a, 4), channel(m, a, i % 2), a, channel(m, a, 5 + hot), channel(m, a, 5 + (hot + 1) % m['C'])):
            c.out[n, ch, h, w] = SATURATED[k % 4]
            k += 1
    for n in range(m['N']):
        for cell in range(1, S * S, 5):          # negatives (and a few positives again): objectness and the IoU prediction
            h, w = divmod(cell, S)
            a = cell % m['an']
            c.out[n, channel(m, a, 4), h, w] = SATURATED[k % 4]
            c.out[n, a, h, w] = SATURATED[(k + 1) % 4]
            k += 1
    return c


SEMANTICS = {
    'wh_tie': wh_tie,
    'xy_tie': xy_tie,
    'identical_square': functools.partial(identical_boxes, True),
    'identical_linear': functools.partial(identical_boxes, False),
    'degenerate': degenerate,
    'disjoint': disjoint,
    'saturation_grid': functools.partial(saturation, 1.05),
    'saturation_plain': functools.partial(saturation, 1.0),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle runs (computed once per case and precision; the results are shared -- do not modify them)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def get(name):
    if name in SEMANTICS:
        return SEMANTICS[name]()
    for shape in GEOMETRY:
        for ia in (False, True):
            if geometry_name(shape, ia) == name:
                return geometry(shape, ia)
    raise KeyError(name)


def _run(case, dtype, term=None):
    out = case.out.to(dtype).clone().requires_grad_(True)
    losses = trn.yolov3_loss([out], [case.target.to(dtype)], case.gt.to(dtype), copy.deepcopy(case.cfg))
    (sum(losses.values()) if term is None else losses[term]).backward()
    return out.grad, {k: (losses[k].detach().double().item() if k in losses else 0.0) for k in LOSS_NAMES}


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float32):
    """train_oracle.yolov3_loss + autograd on case `name` -> (d sum(loss terms) / d out [N, nch, S, S] in `dtype`, {term: value}).
    float32: the reference's arithmetic and tie pattern; float64: every input cast to float64."""
    return _run(get(name), dtype)


def term_grad(name, term):
    """Float32 autograd of ONE loss term (what a tie decides, without the other terms' contributions to the element)."""
    return _run(get(name), torch.float32, term)[0]
