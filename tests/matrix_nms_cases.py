"""Inputs of Matrix-NMS (csrc/decode_nms.hip: nms_sample / nms_collect / nms_select / nms_colmax / nms_decay / nms_finish, with
csrc/nms_select.h) beyond the shipped parameter point, and the oracle runs they are judged by  --  device-free TEST
INFRASTRUCTURE (tests/test_matrix_nms_cases.py checks the builders' own conditions on the CPU, tests/test_gpu_matrix_nms.py runs
the kernels).

A Case holds boxes [N, M, 4], dense scores [N, M, C] (what the oracle sees), the configuration (score_threshold, post_threshold,
nms_top_k, keep_top_k, use_gaussian, sigma; the thresholds are float32 values held as Python floats), `cand_cap` and `meta`.
Where `lists` is None the kernels' candidate list comes from ops.nms_candidates on the dense scores (its order is free: the
entries are appended by atomics).  Otherwise `lists[n] = (key, idx)` are the int32 bit patterns of cand_key / cand_idx of image
n in a CHOSEN order, and `counts[n]` is cand_count; the dense scores are then the ones the stored entries stand for (a list
truncated by cand_cap stands for its first cand_cap entries).  `oracle(name, dtype)` is oracle.ppyolo_oracle.matrix_nms(...,
return_index=True) per image: float32 = the reference's arithmetic, float64 = the inputs cast to float64.

Families (the smallest shapes that still reach the code; scores are a permutation of a float32-exact grid, hence distinct,
unless the family is about ties; boxes are a few dozen base boxes plus jitter so that decay matters):

  topk_*   (nms_top_k, keep_top_k) in TOPK at M = 300, C = 5: `edge` = three images with nms_top_k - 1, nms_top_k and
           nms_top_k + 1 candidates, `many` = 1200 candidates.
  route_*  the list-length routes: the scalar and the 16-byte collect loop (cand_cap = M * 81 odd / M * 80), explicit lists of
           8192 / 8193 entries, all-equal lists of 32768 / 32769 entries, one collect workgroup over its 4096 survivors,
           cand_count beyond cand_cap.  `meta['route']` is what the workspace header must show.
  gauss_*  the Gaussian kernel: sigma in {0.5, 2, 8} x (200, 50) / (1024, 1024), a list above 8192 entries, duplicate boxes
           (comp == 1), a zero-area pair (NaN -> the sentinel).  In float64 every decayed score is at least MARGIN x the largest
           score away from post_threshold and so is the gap at the keep_top_k cut (`margins`; the builders pick the first seed
           for which this holds).
  post_*   a decayed score equal to post_threshold and one float below it; post_threshold = 0 with duplicate boxes; a
           post_threshold above every score.
  index_*  C = 1, 3, 4 with M * C in {4095, 4096, 4097, 4098} (idx_bits 12 / 13), tied top scores at flat index 0 and
           M * C - 1.  (`flat / C` with C = 81 and 80 runs in route_scalar_c81 / route_vector_c80.)
  batch_*  five images in one call: empty, NaN-poisoned, one candidate, a list above 8192, a normal one.
  order_*  one list in three orders: ascending index, descending score, a seeded shuffle.

Not pinned: a score of -0.0 beside +0.0 under a negative threshold.  The order key separates them while the oracle's total order
calls them tied; the model's scores are products of sigmoids and never produce it.
"""
import functools

import numpy as np
import torch

from decode_cases import ERR_FLOOR, RATIO_BOUND, f32      # the constants and the rule of tests/decode_cases.py
from oracle import ppyolo_oracle as orc

KMAX = 1024                  # csrc/nms_select.h
CCAP = 8192                  # candidates the select kernel stages in LDS
NMS_CCAP2 = 32768            # csrc/decode_nms.hip: compact list capacity
NMS_CL = 4096                # survivors one collect workgroup can hold
NMS_CG = 64                  # collect workgroups per image
MARGIN = 1e-5                # float64 distance (x the largest score) the Gaussian builders keep from post_threshold and at the cut
THR = f32(0.01)
TOPK = [(1, 1), (63, 63), (64, 1), (65, 64), (500, 100), (1024, 1024), (1024, 1)]
ORDERS = ['index', 'score', 'shuffle']
NEG_INF = float('-inf')


class Case(object):
    def __init__(self, name, boxes, scores, cfg, cand_cap=None, lists=None, counts=None, tie_free=True, meta=None):
        self.name, self.boxes, self.scores = name, boxes.float().contiguous(), scores.float().contiguous()
        thr, post, topk, keepk, gauss, sigma = cfg
        self.thr, self.post, self.top_k, self.keep_k, self.gauss, self.sigma = \
            f32(thr), f32(post), int(topk), int(keepk), bool(gauss), float(sigma)
        self.cand_cap = self.M * self.C if cand_cap is None else int(cand_cap)
        self.lists, self.counts, self.tie_free, self.meta = lists, counts, tie_free, dict(meta or {})

    @property
    def N(self):
        return self.scores.shape[0]

    @property
    def M(self):
        return self.scores.shape[1]

    @property
    def C(self):
        return self.scores.shape[2]

    @property
    def cfg(self):
        return (self.thr, self.post, self.top_k, self.keep_k, self.gauss, self.sigma)

    def used(self, n):
        """Entries of image n the kernels read: min(cand_count, cand_cap)."""
        if self.lists is None:
            return int((self.scores[n] > self.thr).sum())
        return min(int(self.counts[n]), self.cand_cap)


# ---------------------------------------------------------------------------------------------------------------------------------
# keys and lists
# ---------------------------------------------------------------------------------------------------------------------------------
def score_key(s):
    """include/ppyolo_hip.h: key = bits ^ 0x80000000 for non-negative scores, ~bits for negative ones (float32 array -> uint32)."""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def key_score(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def candidate_list(scores, thr, order, seed=0):
    """(cand_key, cand_idx) of dense scores [M, C] as int32 bit patterns, every entry with score > thr, idx = box * C + class, in
    `order`: 'index' (ascending idx), 'score' (descending score, ties by ascending idx) or 'shuffle' (seeded)."""
    s = scores.detach().cpu().numpy().astype(np.float32).reshape(-1)
    sel = np.nonzero(s > np.float32(thr))[0]
    if order == 'score':
        sel = sel[np.lexsort((sel, -s[sel].astype(np.float64)))]
    elif order == 'shuffle':
        sel = sel[np.random.RandomState(seed).permutation(len(sel))]
    else:
        assert order == 'index'
    return score_key(s[sel]).view(np.int32), sel.astype(np.int32)


def dense_of(key, idx, M, C):
    """The dense scores [M, C] a list stands for: its entries, 0 elsewhere (thresholds here are >= 0, so 0 is no candidate)."""
    s = np.zeros(M * C, dtype=np.float32)
    s[np.asarray(idx, dtype=np.int64)] = key_score(np.asarray(key).view(np.uint32))
    return torch.from_numpy(s).reshape(M, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# ingredients
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _boxes(g, M, nbase=40, jitter=4.0):
    cx, cy = torch.rand(nbase, generator=g) * 640, torch.rand(nbase, generator=g) * 480
    bw, bh = torch.rand(nbase, generator=g) * 160 + 30, torch.rand(nbase, generator=g) * 160 + 30
    base = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    return base[torch.randint(0, nbase, (M,), generator=g)] + torch.randn(M, 4, generator=g) * jitter


def _distinct(g, n, lo, hi):
    """n distinct float32 values: a random permutation of an arithmetic grid."""
    s = torch.linspace(lo, hi, max(n, 2), dtype=torch.float64)[:n][torch.randperm(n, generator=g)].float()
    assert len(torch.unique(s)) == n
    return s


def _dense(g, M, C, count, thr=THR, hi=0.95):
    """Scores [M, C] with exactly `count` entries above thr (distinct, in (thr + 0.01, hi)); the others distinct below thr / 2."""
    total = M * C
    perm = torch.randperm(total, generator=g)
    s = torch.empty(total)
    s[perm[:count]] = _distinct(g, count, thr + 0.01, hi)
    s[perm[count:]] = _distinct(g, total - count, 0.0, thr * 0.5)
    assert int((s > thr).sum()) == count
    return s.reshape(M, C)


def _stack(items):
    return torch.stack([b for b, _ in items]), torch.stack([s for _, s in items])


# ---------------------------------------------------------------------------------------------------------------------------------
# topk_*
# ---------------------------------------------------------------------------------------------------------------------------------
def _topk(topk, keepk, kind):
    g = _gen(1000 + 7 * topk + keepk + (500 if kind == 'many' else 0))
    M, C = 300, 5
    counts = [topk - 1, topk, topk + 1] if kind == 'edge' else [1200]
    b, s = _stack([(_boxes(g, M), _dense(g, M, C, k)) for k in counts])
    return Case('topk_%d_%d_%s' % (topk, keepk, kind), b, s, (THR, 0.01, topk, keepk, False, 2.0), meta=dict(counts=counts))


# ---------------------------------------------------------------------------------------------------------------------------------
# route_*
# ---------------------------------------------------------------------------------------------------------------------------------
def _route_collect(C):
    """Two images through sample + collect with cand_cap = M * C: C = 81 and M odd give an odd capacity (image 1 starts 4 bytes
    off a 16-byte boundary, and whole quads do not fit) = the scalar loop; C = 80 gives the 16-byte loop."""
    g = _gen(2000 + C)
    M = 301
    counts = [M * C, 20000]
    b, s = _stack([(_boxes(g, M), _dense(g, M, C, k)) for k in counts])
    return Case('route_%s_c%d' % ('scalar' if C == 81 else 'vector', C), b, s, (THR, 0.01, 500, 100, False, 2.0),
                meta=dict(counts=counts, route=['compact', 'compact'], scalar=(C == 81)))


def _explicit(name, items, cfg, order, cap=None, cut=None, tie_free=True, meta=None, seed=5):
    """items: (boxes [M, 4], dense scores [M, C]) per image -> a Case whose lists hold the candidates in `order`, cut to `cut`
    entries when given (cand_count stays the full length)."""
    M, C = items[0][1].shape
    lists, counts, dense = [], [], []
    for n, (_, s) in enumerate(items):
        key, idx = candidate_list(s, cfg[0], order, seed + n)
        counts.append(len(key))
        if cut is not None:
            key, idx = key[:cut], idx[:cut]
        lists.append((key, idx))
        dense.append(dense_of(key, idx, M, C))
    return Case(name, torch.stack([b for b, _ in items]), torch.stack(dense), cfg, cand_cap=cap, lists=lists, counts=counts,
                tie_free=tie_free, meta=meta)


def _route_list(count, topk):
    g = _gen(2100 + count + topk)
    M, C = 1100, 8
    route = 'cached' if count <= CCAP else 'compact'
    return _explicit('route_list_%d_k%d' % (count, topk), [(_boxes(g, M), _dense(g, M, C, count))],
                     (THR, 0.01, topk, min(topk, 100), False, 2.0), 'shuffle', meta=dict(counts=[count], route=[route]))


def _route_ties(count):
    """Every entry has ONE value: whatever threshold the sampler picks, the entries at or above it are the whole list."""
    g = _gen(2200 + count)
    M, C = 4100, 8
    s = torch.zeros(M * C)
    s[torch.randperm(M * C, generator=g)[:count]] = 0.5
    route = 'compact_all' if count <= NMS_CCAP2 else 'too_long'
    return _explicit('route_ties_%d' % count, [(_boxes(g, M, nbase=60), s.reshape(M, C))], (THR, 0.01, 500, 100, False, 2.0),
                     'shuffle', tie_free=False, meta=dict(counts=[count], route=[route]))


OVERFLOW_TIES = 5000


def _route_collect_overflow():
    """400 000 entries in ascending index order; OVERFLOW_TIES of them share the highest value and lie inside the slice of one
    collect workgroup (each takes ceil(ceil(count / 4) / 64) quads), everything else is distinct and lower.  About a hundred of
    the sampler's 8192 strata lie wholly inside the tie, far more than the rank it aims at (41), so the threshold is the tied
    value and that workgroup meets 5000 > NMS_CL survivors."""
    g = _gen(2300)
    M, C = 5000, 80
    total = M * C
    per = 4 * (((total + 3) // 4 + NMS_CG - 1) // NMS_CG)
    lo = 3 * per + 500
    assert lo + OVERFLOW_TIES <= 4 * per
    s = _distinct(g, total, 0.02, 0.9)
    s[lo:lo + OVERFLOW_TIES] = 0.95
    return _explicit('route_collect_overflow', [(_boxes(g, M, nbase=60), s.reshape(M, C))], (THR, 0.01, 500, 100, False, 2.0),
                     'index', tie_free=False, meta=dict(counts=[total], route=['overflow'], tie_slice=(lo, lo + OVERFLOW_TIES, per)))


def _route_beyond_cap(count, cap):
    g = _gen(2400 + cap)
    M, C = (1100, 8) if count <= 8800 else (2600, 8)
    items = [(_boxes(g, M), _dense(g, M, C, count)) for _ in range(2)]
    route = 'untouched' if cap <= CCAP else 'compact'
    return _explicit('route_count_%d_cap_%d' % (count, cap), items, (THR, 0.01, 500, 100, False, 2.0), 'shuffle', cap=cap,
                     cut=cap, meta=dict(counts=[count, count], route=[route, route]))


# ---------------------------------------------------------------------------------------------------------------------------------
# gauss_*
# ---------------------------------------------------------------------------------------------------------------------------------
def _all_decayed(c, n, dtype):
    """Every decayed score of image n before post_threshold (NaN ones dropped), descending."""
    rows, _ = orc.matrix_nms(c.boxes[n].to(dtype), c.scores[n].to(dtype), c.thr, NEG_INF, c.top_k, c.top_k, c.gauss, c.sigma,
                             return_index=True)
    return rows[:, 1] if rows[0, 0] >= 0 else rows[:0, 1]


def _margins_of(c):
    """Per image, in float64: (distance of the nearest decayed score to post_threshold, gap at the keep_top_k cut, largest
    score); inf where there is no such score / no cut."""
    out = []
    for n in range(c.N):
        s = _all_decayed(c, n, torch.float64)
        if len(s) == 0:
            out.append((float('inf'), float('inf'), 1.0))
            continue
        kept = s[s >= c.post]
        gap = float(kept[c.keep_k - 1] - kept[c.keep_k]) if len(kept) > c.keep_k else float('inf')
        out.append((float((s - c.post).abs().min()), gap, float(s.max())))
    return out


def _with_margins(build, seed0):
    """The case of the first seed >= seed0 whose float64 decayed scores keep MARGIN from post_threshold and at the cut."""
    for seed in range(seed0, seed0 + 64):
        c = build(seed)
        if all(min(d, gap) >= MARGIN * top for d, gap, top in _margins_of(c)):
            c.meta['seed'] = seed
            return c
    raise AssertionError('no seed with the margins')


def _gauss(sigma, topk, keepk):
    def build(seed):
        g = _gen(seed)
        b, s = _stack([(_boxes(g, 300), _dense(g, 300, 5, 1500)) for _ in range(2)])
        return Case('gauss_s%g_%d_%d' % (sigma, topk, keepk), b, s, (THR, 0.01, topk, keepk, True, sigma))
    return _with_margins(build, 3000 + 100 * int(sigma * 2) + topk)


def _gauss_big_list():
    def build(seed):
        g = _gen(seed)
        b, s = _stack([(_boxes(g, 1100), _dense(g, 1100, 8, 8800)) for _ in range(2)])
        return Case('gauss_big_list', b, s, (THR, 0.01, 200, 50, True, 2.0), meta=dict(route=['compact', 'compact']))
    return _with_margins(build, 3700)


DUPS = [(3, 10), (7, 21), (12, 30)]


def _gauss_dup():
    """Exact duplicate boxes, both classes of each above the threshold: comp == 1 for the lower-scored of a pair."""
    def build(seed):
        g = _gen(seed)
        items = []
        for _ in range(2):
            b = _boxes(g, 60, nbase=12)
            for a, d in DUPS:
                b[d] = b[a]
            items.append((b, _dense(g, 60, 2, 120)))
        b, s = _stack(items)
        return Case('gauss_dup', b, s, (THR, 0.01, 200, 50, True, 2.0))
    return _with_margins(build, 3800)


def _zero_area(b):
    b[5] = torch.tensor([100., 100., 100., 150.])
    b[9] = torch.tensor([300., 200., 300., 200.])


def _gauss_nan():
    """Image 0 holds two zero-area boxes (0 / 0 IoU: every decay is NaN, the sentinel); image 1 is an ordinary neighbour."""
    def build(seed):
        g = _gen(seed)
        b, s = _stack([(_boxes(g, 60, nbase=12), _dense(g, 60, 2, 120)) for _ in range(2)])
        _zero_area(b[0])
        return Case('gauss_nan', b, s, (THR, 0.01, 200, 50, True, 2.0), meta=dict(nan_images=[0]))
    return _with_margins(build, 3900)


# ---------------------------------------------------------------------------------------------------------------------------------
# post_*
# ---------------------------------------------------------------------------------------------------------------------------------
POST_P = f32(0.25)


def _post_equal_below():
    """Boxes 118 and 119 are far from everything and are the only members of classes 2 and 3: their decay coefficient is exactly
    1.  Box 118 scores post_threshold itself (kept, >=), box 119 the float32 just below it (dropped)."""
    g = _gen(4000)
    M, C = 120, 4
    b = _boxes(g, M, nbase=12)
    b[118] = torch.tensor([5000., 5000., 5100., 5100.])
    b[119] = torch.tensor([7000., 7000., 7100., 7100.])
    s = torch.zeros(M, C)
    s[:118, :2] = _dense(g, 118, 2, 236)
    below = float(np.nextafter(np.float32(POST_P), np.float32(0)))
    s[118, 2], s[119, 3] = POST_P, below
    return Case('post_equal_below', b[None], s[None], (THR, POST_P, 500, 500, False, 2.0),
                meta=dict(equal=118 * C + 2, below=119 * C + 3, below_score=below))


def _post_zero_dups():
    """post_threshold = 0 with three duplicated boxes: the lower-scored copy of each (in both classes) decays to exactly 0.0, is
    kept (0 >= 0), and the six zeros come out in first-sort order."""
    g = _gen(4100)
    b = _boxes(g, 40, nbase=8)
    for a, d in DUPS:
        b[d] = b[a]
    return Case('post_zero_dups', b[None], _dense(g, 40, 2, 80)[None], (THR, 0.0, 500, 500, False, 2.0), tie_free=False,
                meta=dict(zeros=2 * len(DUPS)))


def _post_above_all():
    g = _gen(4200)
    return Case('post_above_all', _boxes(g, 300)[None], _dense(g, 300, 5, 1200)[None], (THR, 0.99, 500, 100, False, 2.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# index_*
# ---------------------------------------------------------------------------------------------------------------------------------
INDEX_SHAPES = {'index_c1_4096': (4096, 1), 'index_c1_4097': (4097, 1), 'index_c3_4095': (1365, 3), 'index_c3_4098': (1366, 3),
                'index_c4_4096': (1024, 4)}


def _index(name):
    """The two highest scores are equal and sit at flat index 0 and M * C - 1, on two boxes far from everything (both survive
    undecayed: flat 0 comes first).  M * C = 4096 is exactly 2^12 (idx_bits 12), 4097 / 4098 take 13 bits.  4096 is no
    multiple of 3: C = 1 and C = 4 hit it, C = 3 straddles it with 4095 and 4098."""
    M, C = INDEX_SHAPES[name]
    g = _gen(5000 + M * C)
    b = _boxes(g, M)
    b[0] = torch.tensor([5000., 5000., 5100., 5100.])
    b[M - 1] = torch.tensor([7000., 7000., 7100., 7100.])
    s = _dense(g, M, C, 1200, hi=0.9).reshape(-1)
    s[0], s[M * C - 1] = 0.95, 0.95
    return Case(name, b[None], s.reshape(1, M, C), (THR, 0.01, 500, 100, False, 2.0), tie_free=False,
                meta=dict(first=0, last=M * C - 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# batch_*
# ---------------------------------------------------------------------------------------------------------------------------------
BATCH_KINDS = ['empty', 'nan', 'one', 'large', 'normal']


def _batch(gauss):
    def build(seed):
        g = _gen(seed)
        M, C = 1100, 8
        items = [(_boxes(g, M), _dense(g, M, C, k)) for k in (0, 300, 1, M * C, 1200)]
        s = items[1][1]
        s[5, 0], s[9, 0] = 0.5, 0.4              # the two zero-area boxes are candidates
        _zero_area(items[1][0])
        b, s = _stack(items)
        return Case('batch_%s' % ('gauss' if gauss else 'linear'), b, s, (THR, 0.01, 500, 100, gauss, 2.0),
                    meta=dict(kinds=BATCH_KINDS, route=['cached', 'cached', 'cached', 'compact', 'cached'], nan_images=[1]))
    return _with_margins(build, 6000) if gauss else build(6000)


def take(case, images, name):
    """The case made of `images` (indices, repeats allowed) of a dense-score case."""
    assert case.lists is None
    images = list(images)
    meta = dict(case.meta, source=case.name, images=images)
    if 'route' in case.meta:
        meta['route'] = [case.meta['route'][i] for i in images]
    return Case(name, case.boxes[images], case.scores[images], case.cfg, cand_cap=case.cand_cap, tie_free=case.tie_free, meta=meta)


# ---------------------------------------------------------------------------------------------------------------------------------
# order_*
# ---------------------------------------------------------------------------------------------------------------------------------
def _order(family, order):
    g = _gen(7000 + len(family))
    route = None
    if family == 'small':
        items, tie_free = [(_boxes(g, 300), _dense(g, 300, 5, 1200))], True
    elif family == 'large':
        items, tie_free, route = [(_boxes(g, 1100), _dense(g, 1100, 8, 8800))], True, ['compact']
    else:
        b = _boxes(g, 700)
        items, tie_free = [(b, torch.randint(1, 40, (700, 3), generator=g).float() / 64.0)], False
    return _explicit('order_%s_%s' % (family, order), items, (f32(0.05) if family == 'ties' else THR, 0.01, 500, 100, False, 2.0),
                     order, tie_free=tie_free, meta=dict(family=family, order=order, **({'route': route} if route else {})))


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases and their oracle runs (computed once per case and precision; the results are shared -- do not modify them)
# ---------------------------------------------------------------------------------------------------------------------------------
BUILDERS = {}
for _t, _k in TOPK:
    for _kind in ('edge', 'many'):
        BUILDERS['topk_%d_%d_%s' % (_t, _k, _kind)] = functools.partial(_topk, _t, _k, _kind)
BUILDERS['route_scalar_c81'] = functools.partial(_route_collect, 81)
BUILDERS['route_vector_c80'] = functools.partial(_route_collect, 80)
for _n in (CCAP, CCAP + 1):
    for _t in (1024, 100):
        BUILDERS['route_list_%d_k%d' % (_n, _t)] = functools.partial(_route_list, _n, _t)
for _n in (NMS_CCAP2, NMS_CCAP2 + 1):
    BUILDERS['route_ties_%d' % _n] = functools.partial(_route_ties, _n)
BUILDERS['route_collect_overflow'] = _route_collect_overflow
BUILDERS['route_count_7000_cap_5000'] = functools.partial(_route_beyond_cap, 7000, 5000)
BUILDERS['route_count_20000_cap_9000'] = functools.partial(_route_beyond_cap, 20000, 9000)
SIGMAS = [0.5, 2.0, 8.0]
for _s in SIGMAS:
    for _t, _k in ((200, 50), (1024, 1024)):
        BUILDERS['gauss_s%g_%d_%d' % (_s, _t, _k)] = functools.partial(_gauss, _s, _t, _k)
BUILDERS['gauss_big_list'] = _gauss_big_list
BUILDERS['gauss_dup'] = _gauss_dup
BUILDERS['gauss_nan'] = _gauss_nan
BUILDERS['post_equal_below'] = _post_equal_below
BUILDERS['post_zero_dups'] = _post_zero_dups
BUILDERS['post_above_all'] = _post_above_all
for _n in INDEX_SHAPES:
    BUILDERS[_n] = functools.partial(_index, _n)
BUILDERS['batch_linear'] = functools.partial(_batch, False)
BUILDERS['batch_gauss'] = functools.partial(_batch, True)
ORDER_FAMILIES = ['small', 'large', 'ties']
for _f in ORDER_FAMILIES:
    for _o in ORDERS:
        BUILDERS['order_%s_%s' % (_f, _o)] = functools.partial(_order, _f, _o)


def names(prefix=''):
    return sorted(n for n in BUILDERS if n.startswith(prefix))


def golden_names():
    """The tie-free cases the reference itself has an answer for (one order of each order_* family: the dense scores are the same)."""
    return [n for n in names() if get(n).tie_free and not (n.startswith('order_') and not n.endswith('_index'))]


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()


def run_oracle(case, n, dtype):
    """-> (rows [k, 6], keep indices int64 [k]) of image n; k == 0 stands for the reference's sentinel."""
    rows, keep = orc.matrix_nms(case.boxes[n].to(dtype), case.scores[n].to(dtype), case.thr, case.post, case.top_k, case.keep_k,
                                case.gauss, case.sigma, return_index=True)
    if rows[0, 0] < 0:
        return rows[:0], np.zeros((0,), np.int64)
    return rows, np.asarray(keep, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float32):
    """-> per image (rows [k, 6], keep [k]) of case `name` in `dtype`."""
    c = get(name)
    return [run_oracle(c, n, dtype) for n in range(c.N)]


@functools.lru_cache(maxsize=None)
def margins(name):
    return _margins_of(get(name))


def score_errors(name, n, keep, scores):
    """Gaussian rule for image n: `scores` (float32, any order) matched to the oracles by `keep` index -> (largest |score -
    score64|, the float32 oracle's own largest error, the floor ERR_FLOOR x the largest score).  The kept sets must be equal."""
    r64, k64 = oracle(name, torch.float64)[n]
    r32, k32 = oracle(name, torch.float32)[n]
    ref = dict(zip(k64.tolist(), r64[:, 1].tolist()))
    own = dict(zip(k32.tolist(), r32[:, 1].double().tolist()))
    assert set(ref) == set(own) == set(np.asarray(keep).tolist())
    if not ref:
        return 0.0, 0.0, 0.0
    err = max(abs(float(s) - ref[k]) for k, s in zip(np.asarray(keep).tolist(), np.asarray(scores, dtype=np.float64).tolist()))
    e32 = max(abs(own[k] - ref[k]) for k in ref)
    return err, e32, ERR_FLOOR * max(ref.values())


def bound_of(e32, floor):
    return RATIO_BOUND * max(e32, floor)
