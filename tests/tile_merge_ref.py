"""float32 numpy restatement of the cross-view merge of tiled inference (csrc/merge_views.hip, include/ppyolo_hip.h), the tile
grid rule restated independently of ppyolo_hip/tiles.py, and the cases shared by tests/test_tile_merge_ref.py (hand-derived
answers, fairness of the seeded cases) and tests/test_gpu_tile_merge.py (bit-for-bit comparison).

    admission:   row r of view v iff r < min(count[v], K), all six values finite, 0 <= class < 2^24, score >= score_thresh;
                 the class id is the truncated value; a view whose image is -1 is padding and ignored
    translation: x0, x1 += float32(ox), y0, y1 += float32(oy), one float32 rounding each, no clipping
    order:       per image: score descending as values (-0.0 ties with +0.0), then view ascending, then row ascending
    scan:        greedy: a candidate is selected iff metric(candidate, k) <= thresh for every already selected k (of the same
                 class id unless class_agnostic); a NaN metric suppresses
    metric:      'iou' = multiclass_nms_ref.iou, normalized; 'ios' = the same disjoint rule, iw, ih and inter, then
                 inter / (area_k < area_candidate ? area_k : area_candidate)
    output:      the first keep_top_k selections in scan order; -1 padding

Everything stays in np.float32 arrays (numpy rounds each elementwise operation once; nothing here can fuse)."""
import numpy as np

from multiclass_nms_ref import area, clustered, iou

F = np.float32


def ios(a, b):
    """Intersection over the smaller box: one box a [4] with boxes b [K, 4], float32 -> float32 [K]."""
    a = np.asarray(a, dtype=F)
    b = np.asarray(b, dtype=F)
    norm = F(0)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        disjoint = (b[..., 0] > a[2]) | (b[..., 2] < a[0]) | (b[..., 1] > a[3]) | (b[..., 3] < a[1])
        x2 = np.where(b[..., 2] < a[2], b[..., 2], a[2])
        x1 = np.where(a[0] < b[..., 0], b[..., 0], a[0])
        y2 = np.where(b[..., 3] < a[3], b[..., 3], a[3])
        y1 = np.where(a[1] < b[..., 1], b[..., 1], a[1])
        iw = ((x2 - x1).astype(F) + norm).astype(F)
        ih = ((y2 - y1).astype(F) + norm).astype(F)
        inter = (iw * ih).astype(F)
        aa, ab = area(a, norm), area(b, norm)
        out = (inter / np.where(ab < aa, ab, aa).astype(F)).astype(F)
    return np.where(disjoint, F(0), out).astype(F)


def metric_fn(metric):
    if metric == 'iou':
        return lambda a, b: iou(a, b, normalized=True)
    if metric == 'ios':
        return ios
    raise ValueError('unknown metric %r' % (metric,))


def admitted_rows(dets, count, views, image, score_thresh):
    """[(view, row)] of one image, in table order."""
    dets = np.asarray(dets, dtype=F)
    V, K = dets.shape[0], dets.shape[1]
    out = []
    with np.errstate(invalid='ignore'):
        for v in range(V):
            if int(views[v][0]) != image:
                continue
            for r in range(max(0, min(int(count[v]), K))):
                row = dets[v, r]
                if not np.all(np.isfinite(row)):
                    continue
                if not (row[0] >= F(0) and row[0] < F(16777216.0) and row[1] >= F(score_thresh)):
                    continue
                out.append((v, r))
    return out


def merge_image(dets, count, views, image, metric='ios', thresh=0.5, score_thresh=0.0, class_agnostic=False, stats=None):
    """Every selection of one image in scan order, before the keep_top_k cut: ([(view, row)], translated boxes float32 [k, 4])."""
    dets = np.asarray(dets, dtype=F)
    views = np.asarray(views)
    fn, thr = metric_fn(metric), F(thresh)
    adm = admitted_rows(dets, count, views, image, score_thresh)
    if adm:
        vv = np.array([a[0] for a in adm])
        rr = np.array([a[1] for a in adm])
        sc = dets[vv, rr, 1].astype(np.float64)
        order = np.lexsort((rr, vv, -sc))                          # score descending by value, view ascending, row ascending
        off = np.stack([views[vv, 1], views[vv, 2], views[vv, 1], views[vv, 2]], axis=1).astype(F)      # float32(ox): one rounding
        with np.errstate(over='ignore', invalid='ignore'):
            boxes = (dets[vv, rr, 2:6] + off).astype(F)
        cls = dets[vv, rr, 0].astype(np.int64)                    # truncation
    else:
        order = np.zeros((0,), dtype=np.int64)
    kept, kb, kc = [], np.zeros((len(adm), 4), dtype=F), np.zeros((len(adm),), dtype=np.int64)
    for i in order:
        ok = True
        if kept:
            m = fn(boxes[i], kb[:len(kept)])
            bad = ~(m <= thr)                                      # NaN <= thr is False: suppressed
            if not class_agnostic:
                bad &= kc[:len(kept)] == cls[i]
            ok = not bool(np.any(bad))
        if ok:
            kb[len(kept)] = boxes[i]
            kc[len(kept)] = cls[i]
            kept.append(int(i))
    if stats is not None:
        stats.update(admitted=len(adm), selected=len(kept), suppressed=len(adm) - len(kept))
    return [adm[i] for i in kept], kb[:len(kept)].copy()


def padded(dets, selections, keep_top_k):
    """[(src, boxes)] per image (merge_image's results) -> (out_dets [n, keep_top_k, 6], out_count [n], out_src [n, keep_top_k, 2])
    as the kernel writes them: the first keep_top_k selections, -1 behind them."""
    dets = np.asarray(dets, dtype=F)
    n = len(selections)
    od = np.full((n, keep_top_k, 6), -1, dtype=F)
    oc = np.zeros((n,), dtype=np.int32)
    osrc = np.full((n, keep_top_k, 2), -1, dtype=np.int32)
    for i, (src, boxes) in enumerate(selections):
        k = min(len(src), keep_top_k)
        oc[i] = k
        for j in range(k):
            v, r = src[j]
            od[i, j, 0:2] = dets[v, r, 0:2]
            od[i, j, 2:6] = boxes[j]
            osrc[i, j] = (v, r)
    return od, oc, osrc


def merge_views(dets, count, views, n, metric='ios', thresh=0.5, score_thresh=0.0, class_agnostic=False, keep_top_k=100, stats=None):
    """The whole call.  stats (a list, optional) receives one dict per image."""
    sel = []
    for i in range(n):
        st = {} if stats is not None else None
        sel.append(merge_image(dets, count, views, i, metric, thresh, score_thresh, class_agnostic, st))
        if stats is not None:
            stats.append(st)
    return padded(dets, sel, keep_top_k)


# ---- the tile grid, restated --------------------------------------------------------------------------------------------------

def grid_origins(L, T, overlap):
    if L <= T:
        return [0], L
    s = max(1, int(np.floor(T * (1 - overlap))))
    o = list(range(0, L - T, s))              # 0, s, 2s, ... while o + T < L
    return o + [L - T], T


def grid_views(h, w, tile, overlap, full_view):
    xs, vw = grid_origins(w, tile, overlap)
    ys, vh = grid_origins(h, tile, overlap)
    tiles = [(ox, oy, vw, vh) for oy in ys for ox in xs]
    return ([(0, 0, w, h)] if full_view and len(tiles) > 1 else []) + tiles


GRID_VALUES = [((608, 608, .2), [0]), ((609, 608, .2), [0, 1]), ((1000, 608, .2), [0, 392]),
               ((3840, 608, .2), [0, 486, 972, 1458, 1944, 2430, 2916, 3232]), ((2160, 608, .2), [0, 486, 972, 1458, 1552]),
               ((640, 192, .2), [0, 153, 306, 448]), ((418, 192, .2), [0, 153, 226]), ((129, 64, 0), [0, 64, 65]),
               ((200, 64, .5), [0, 32, 64, 96, 128, 136])]


# ---- the shared cases ---------------------------------------------------------------------------------------------------------
# A case is a dict: dets [V, K, 6], count [V], views [V, 3], n, and `kw` = the call's parameters.

def case(rows_per_view, views, n, K=None, count=None, **kw):
    """rows_per_view: per view a list of (class, score, x0, y0, x1, y1); rows behind a view's list are filled with a row that
    would be admitted (class 0, score 0.99, a box of its own), so that a kernel reading past count shows."""
    V = len(rows_per_view)
    K = max(len(r) for r in rows_per_view) if K is None else K
    dets = np.zeros((V, K, 6), dtype=F)
    for v in range(V):
        for r in range(K):
            dets[v, r] = (0, 0.99, 5000 + 40 * v, 5000 + 40 * r, 5030 + 40 * v, 5030 + 40 * r)
        for r, row in enumerate(rows_per_view[v]):
            dets[v, r] = row
    cnt = np.array([len(r) for r in rows_per_view] if count is None else count, dtype=np.int32)
    params = dict(metric='ios', thresh=0.5, score_thresh=0.0, class_agnostic=False, keep_top_k=8)
    params.update(kw)
    return dict(dets=dets, count=cnt, views=np.array(views, dtype=np.int32).reshape(V, 3), n=n, kw=params)


def halves(whole, left, right, **kw):
    """One object [100, 100, 300, 200] seen whole by the full view, its left half by the tile at (0, 50), its right half by the
    tile at (200, 50)."""
    return case([[(1, whole, 100, 100, 300, 200)], [(1, left, 100, 50, 200, 150)], [(1, right, 0, 50, 100, 150)]],
                [(0, 0, 0), (0, 0, 50), (0, 200, 50)], 1, **kw)


NAN, INF = float('nan'), float('inf')


def hand_cases():
    c = {}
    c['halves_ios'] = halves(.9, .8, .7)
    c['halves_iou'] = halves(.9, .8, .7, metric='iou')
    c['halves_reversed_ios'] = halves(.7, .9, .8)
    # equal scores: view order, then row order; the views of image 0 are table entries 2 and 0, image 1 has entry 1
    c['equal_scores'] = case([[(0, .5, 0, 0, 10, 10), (0, .5, 20, 0, 30, 10)], [(0, .5, 0, 0, 10, 10)],
                              [(0, .5, 40, 0, 50, 10), (0, .5, 60, 0, 70, 10)]], [(0, 0, 0), (1, 7, 9), (0, 0, 100)], 2)
    # the +0.0 comes LAST in (view, row) order: ordering the bit patterns would put it first
    c['signed_zero'] = case([[(0, -0.0, 0, 0, 10, 10), (0, -0.0, 20, 0, 30, 10), (0, -.5, 80, 0, 90, 10)], [(0, 0.0, 40, 0, 50, 10)]],
                             [(0, 0, 0), (0, 0, 0)], 1, score_thresh=-1.0)
    same = [[(1, .9, 10, 10, 50, 50), (2, .8, 10, 10, 50, 50)]]
    c['classes_aware'] = case(same, [(0, 3, 4)], 1)
    c['classes_agnostic'] = case(same, [(0, 3, 4)], 1, class_agnostic=True)
    # class 2.5 is class id 2: it meets the class-2 row at the same place
    c['truncated_class'] = case([[(2, .9, 10, 10, 50, 50), (2.5, .8, 10, 10, 50, 50), (3.5, .7, 10, 10, 50, 50)]], [(0, 0, 0)], 1)
    # left out: a NaN, an inf, a negative class, class 2^24, a score below the threshold, the row at r == count (view 0 holds a
    # third row); view 1 says count = 5 with K = 3: its three rows are read, nothing more
    c['left_out'] = case([[(0, .9, 0, 0, 10, 10), (0, .8, 20, NAN, 30, 10), (0, .7, 100, 0, 110, 10)],
                          [(0, INF, 200, 0, 210, 10), (-1, .8, 220, 0, 230, 10), (16777216.0, .8, 240, 0, 250, 10)],
                          [(0, .3, 300, 0, 310, 10), (16777215.0, .6, 320, 0, 330, 10), (0, .29, 340, 0, 350, 10)]],
                         [(0, 0, 0), (0, 0, 0), (0, 0, 0)], 1, count=[2, 3, 5], score_thresh=0.3)
    # a padding view with the best scores, between the views of the image
    c['padding_view'] = case([[(0, .5, 0, 0, 10, 10)], [(0, .9, 0, 0, 10, 10)], [(0, .6, 0, 0, 10, 10)]],
                             [(0, 0, 0), (-1, 0, 0), (0, 100, 0)], 1)
    zero = [[(0, .9, 10, 10, 10, 20), (0, .8, 10, 10, 10, 20), (0, .7, 5, 5, 15, 25)]]
    c['zero_area_iou'] = case(zero, [(0, 0, 0)], 1, metric='iou')
    c['zero_area_ios'] = case(zero, [(0, 0, 0)], 1)
    c['thresh_one_iou'] = case([[(1, .9, 100, 100, 300, 200), (1, .6, 100, 100, 300, 200)], [(1, .8, 100, 50, 200, 150)],
                                [(1, .7, 0, 50, 100, 150), (1, .95, 0, 50, 100, 150)]],
                               [(0, 0, 0), (0, 0, 50), (0, 200, 50)], 1, metric='iou', thresh=1.0)
    c['cut'] = case([[(0, .5 + .01 * i, 20 * i, 0, 20 * i + 10, 10) for i in range(3)], [(0, .7 + .01 * i, 20 * i, 0, 20 * i + 10, 10) for i in range(2)]],
                    [(0, 0, 0), (0, 0, 100)], 1, keep_top_k=3)
    return c


MODES = [('iou', False), ('iou', True), ('ios', False), ('ios', True)]
SEEDS = (0, 1, 2, 3)
# selections of the four modes on clustered(seed, M=700, C=5), class = argmax, score = max, admitted at 0.3, thresh 0.5
MODE_COUNTS = {0: (92, 27, 63, 14), 1: (89, 23, 52, 13), 2: (95, 29, 57, 12), 3: (86, 23, 56, 13)}


def clustered_rows(seed, M=700, centres=12):
    """The recipe's boxes as rows: class = argmax of the scores, score = their max."""
    boxes, scores = clustered(seed, M=M, C=5, centres=centres)
    return np.concatenate([scores.argmax(axis=1)[:, None].astype(F), scores.max(axis=1)[:, None], boxes], axis=1).astype(F)


def flat_case(seed, **kw):
    """The recipe as it stands: one view at (0, 0) holding all 700 rows."""
    rows = clustered_rows(seed)
    params = dict(metric='ios', thresh=0.5, score_thresh=0.3, class_agnostic=False, keep_top_k=1024)
    params.update(kw)
    return dict(dets=rows[None], count=np.array([rows.shape[0]], dtype=np.int32), views=np.zeros((1, 3), dtype=np.int32), n=1, kw=params)


# (V, K) of the spread cases.  A case holds min(700, V * K) rows of the recipe, dealt to the views at random (so the views are
# unevenly filled unless the case is full), each view at a random integer offset, the row stored in view coordinates.
SPREAD = [(1, 100), (2, 7), (2, 100), (5, 7), (5, 100), (41, 1), (41, 7), (41, 100)]
KEEPS = (1, 40, 1024)


def spread_case(seed, V, K, image=0, n=1):
    M = min(700, V * K)
    rows = clustered_rows(seed, M=M, centres=max(1, min(12, M // 6)))
    r = np.random.RandomState(1000 + seed)
    view_of = r.permutation(np.repeat(np.arange(V), K))[:M]
    off = np.stack([r.randint(-50, 3000, size=V), r.randint(-50, 3000, size=V)], axis=1)
    dets = np.zeros((V, K, 6), dtype=F)
    dets[:, :, :] = np.array([0, 0.99, 1, 1, 31, 31], dtype=F)        # behind count: rows that would be admitted
    count = np.zeros((V,), dtype=np.int32)
    for i in range(M):
        v = view_of[i]
        row = rows[i].copy()
        row[2:6] = (row[2:6] - np.array([off[v, 0], off[v, 1], off[v, 0], off[v, 1]], dtype=F)).astype(F)
        dets[v, count[v]] = row
        count[v] += 1
    views = np.concatenate([np.full((V, 1), image), off], axis=1).astype(np.int32)
    return dict(dets=dets, count=count, views=views, n=n,
                kw=dict(metric='ios', thresh=0.5, score_thresh=0.3, class_agnostic=False, keep_top_k=1024))


def uniform_case(R, V, K, seed=7):
    """R = V * K rows, every one admitted, in one image: boxes of 20..80 px placed uniformly in a square of 22 sqrt(R) px (2000
    for 8192 rows: a box meets a handful of others at every R), scores on a grid of 1/256 so that many tie, five classes.  For the boundaries of the kernel's stages."""
    assert R == V * K
    r = np.random.RandomState(seed + R)
    ctr = r.uniform(0, 22.0 * np.sqrt(R), size=(R, 2))
    size = r.uniform(20, 80, size=(R, 2))
    off = np.stack([r.randint(0, 500, size=V), r.randint(0, 500, size=V)], axis=1)
    dets = np.zeros((V, K, 6), dtype=F)
    dets[:, :, 0] = r.randint(0, 5, size=(V, K))
    dets[:, :, 1] = (r.randint(77, 256, size=(V, K)) / 256.0).astype(F)
    dets[:, :, 2:4] = (ctr - size / 2).reshape(V, K, 2) - off[:, None, :]
    dets[:, :, 4:6] = (ctr + size / 2).reshape(V, K, 2) - off[:, None, :]
    views = np.concatenate([np.zeros((V, 1)), off], axis=1).astype(np.int32)
    return dict(dets=dets, count=np.full((V,), K, dtype=np.int32), views=views, n=1,
                kw=dict(metric='iou', thresh=0.3, score_thresh=0.3, class_agnostic=True, keep_top_k=1024))


# rows per image at the kernel's stage boundaries: (R, V, K).  CHUNK = 64 candidates per scan step, RANK_MAX = 1024 rows the
# counting sort orders (beyond: the bitonic network), MAX_ROWS = 8192 the keys' stage.
CHUNK, RANK_MAX, MAX_ROWS = 64, 1024, 8192
BOUNDARIES = [(63, 9, 7), (64, 8, 8), (65, 13, 5), (1023, 33, 31), (1024, 32, 32), (1025, 25, 41), (8192, 64, 128)]
TOO_MANY = (8193, 3, 2731)


def concat_cases(cases, order=None):
    """Several one-image cases (same K) as one batch: image i = case i; `order` = the table's order as (case, view) pairs
    (default: case after case).  The parameters are the first case's."""
    K = cases[0]['dets'].shape[1]
    assert all(c['dets'].shape[1] == K and c['n'] == 1 for c in cases)
    if order is None:
        order = [(i, v) for i, c in enumerate(cases) for v in range(c['dets'].shape[0])]
    dets = np.stack([cases[i]['dets'][v] for i, v in order])
    count = np.array([cases[i]['count'][v] for i, v in order], dtype=np.int32)
    views = np.array([[i if cases[i]['views'][v][0] >= 0 else -1, cases[i]['views'][v][1], cases[i]['views'][v][2]] for i, v in order],
                     dtype=np.int32)
    return dict(dets=dets, count=count, views=views, n=len(cases), kw=dict(cases[0]['kw']))


def interleaved_case():
    """The views of two images alternating in the table."""
    a, b = spread_case(0, 5, 100), spread_case(1, 5, 100)
    return concat_cases([a, b], [(i, v) for v in range(5) for i in (0, 1)])


def batch_case():
    """Image 0: views, but no admitted row; image 1: nothing but padding views; image 2: full (MAX_ROWS rows, all admitted)."""
    full = uniform_case(8192, 64, 128)
    low = uniform_case(256, 2, 128, seed=11)
    low['dets'][:, :, 1] = F(0.1)
    pad = uniform_case(384, 3, 128, seed=12)
    pad['views'][:, 0] = -1
    return concat_cases([low, pad, full], [(0, 0), (1, 0), (2, 0)] + [(2, v) for v in range(1, 64)] + [(1, 1), (0, 1), (1, 2)])


def run(c, **kw):
    """The restatement on a case, with parameters overridden."""
    params = dict(c['kw'])
    params.update(kw)
    return merge_views(c['dets'], c['count'], c['views'], c['n'], **params)
