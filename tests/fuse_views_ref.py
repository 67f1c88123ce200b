"""float32 numpy restatement of the weighted boxes fusion across views (csrc/fuse_views.hip, include/ppyolo_hip.h), and the cases
shared by tests/test_fuse_views_ref.py (hand-derived answers, what the seeded cases exercise) and tests/test_gpu_fuse_views.py
(bit-for-bit comparison).

    transform:   mirror_w > 0: nx0 = float32(mirror_w) - x1, nx1 = float32(mirror_w) - x0; then x += float32(ox), y += float32(oy)
    admission:   row r of view v iff r < min(count[v], K), all six values finite, 0 <= class < 2^24, score >= score_thresh,
                 score > 0, and the transformed box has x1 > x0 and y1 > y0; a view whose image is -1 is padding and ignored
    order:       per image: s = score * weight[v] descending, then view ascending, then row ascending
    clusters:    per class id, rows in that order: iou(row, fused box of every cluster); the largest STRICTLY above thresh joins
                 (the earliest cluster on a tie, NaN never): S += s, X += s * b, T += 1, fused = X / S; else a new cluster with
                 S = s, X = s * b, T = 1, fused = the row's box
    confidence:  wsum = sum of weight over the image's views in table order; q = S / T, m = min(T, wsum), conf = (q * m) / wsum
    output:      conf descending, class ascending, creation order; the first keep_top_k; -1 padding

Every scalar is an np.float32 and every array float32, so each operation rounds once to float32 (a Python float or a float64
anywhere in a running sum would not)."""
import numpy as np

import tile_merge_ref as T
from multiclass_nms_ref import iou

F = np.float32
MAX_ROWS, RANK_MAX = T.MAX_ROWS, T.RANK_MAX


def transform(row, view):
    """row [6] float32, view = (image, ox, oy, mirror_w) -> the box in image coordinates, float32 [4]."""
    x0, y0, x1, y1 = F(row[2]), F(row[3]), F(row[4]), F(row[5])
    mw = int(view[3])
    with np.errstate(over='ignore', invalid='ignore'):
        if mw > 0:
            w = F(mw)
            x0, x1 = F(w - x1), F(w - x0)
        ox, oy = F(int(view[1])), F(int(view[2]))
        return np.array([F(x0 + ox), F(y0 + oy), F(x1 + ox), F(y1 + oy)], dtype=F)


def admitted_rows(dets, count, views, image, score_thresh):
    """[(view, row, box)] of one image, in table order."""
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
                if not (row[0] >= F(0) and row[0] < F(16777216.0) and row[1] >= F(score_thresh) and row[1] > F(0)):
                    continue
                b = transform(row, views[v])
                if not (b[2] > b[0] and b[3] > b[1]):
                    continue
                out.append((v, r, b))
    return out


def weight_sum(views, weight, image):
    w = F(0)
    for v in range(len(views)):
        if int(views[v][0]) == image:
            w = F(w + F(weight[v]))
    return w


def fuse_image(dets, count, views, weight, image, thresh=0.55, score_thresh=0.0, stats=None):
    """Every cluster of one image in output order, before the keep_top_k cut: a list of (class id, conf float32, fused box
    float32 [4], (view, row) of the first member, members)."""
    dets = np.asarray(dets, dtype=F)
    views = np.asarray(views)
    weight = np.asarray(weight, dtype=F)
    thr = F(thresh)
    adm = admitted_rows(dets, count, views, image, score_thresh)
    wsum = weight_sum(views, weight, image)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        s_of = [F(dets[v, r, 1] * weight[v]) for v, r, _ in adm]
        order = sorted(range(len(adm)), key=lambda i: (-float(s_of[i]), adm[i][0], adm[i][1]))
        per_class = {}
        for i in order:
            per_class[int(dets[adm[i][0], adm[i][1], 0])] = per_class.get(int(dets[adm[i][0], adm[i][1], 0]), 0) + 1
        state = {c: dict(n=0, fused=np.zeros((m, 4), dtype=F), X=np.zeros((m, 4), dtype=F), S=np.zeros((m,), dtype=F),
                         T=np.zeros((m,), dtype=np.int64), first=[None] * m, born=[0] * m) for c, m in per_class.items()}
        born = 0
        for i in order:
            v, r, b = adm[i]
            s = s_of[i]
            st = state[int(dets[v, r, 0])]
            k = st['n']
            c = -1
            if k:
                m = iou(b, st['fused'][:k], normalized=True)
                ok = m > thr                                       # NaN > thr is False
                if ok.any():
                    c = int(np.argmax(np.where(ok, m, F(-np.inf))))      # the first of equal maxima
            if c >= 0:
                st['S'][c] = F(st['S'][c] + s)
                st['X'][c] = (st['X'][c] + (s * b).astype(F)).astype(F)
                st['T'][c] += 1
                st['fused'][c] = (st['X'][c] / st['S'][c]).astype(F)
            else:
                st['S'][k] = s
                st['X'][k] = (s * b).astype(F)
                st['T'][k] = 1
                st['fused'][k] = b                                 # bit for bit
                st['first'][k] = (v, r)
                st['born'][k] = born
                st['n'] = k + 1
                born += 1
        out = []
        for c, st in state.items():
            for k in range(st['n']):
                tf = F(st['T'][k])
                q = F(st['S'][k] / tf)
                m = wsum if wsum < tf else tf
                conf = F(F(q * m) / wsum)
                out.append((c, conf, st['fused'][k].copy(), st['first'][k], int(st['T'][k]), st['born'][k]))
    out.sort(key=lambda t: (-float(t[1]), t[0], t[5]))
    if stats is not None:
        members = [t[4] for t in out]
        stats.update(admitted=len(adm), clusters=len(out), max_members=max(members) if members else 0,
                     singletons=sum(1 for t in members if t == 1), classes=len(state))
    return [t[:5] for t in out]


def padded(clusters, keep_top_k):
    """[clusters of an image] -> (out_dets [n, k, 6], out_count [n], out_src [n, k, 2], out_members [n, k]) as the kernel writes."""
    n = len(clusters)
    od = np.full((n, keep_top_k, 6), -1, dtype=F)
    oc = np.zeros((n,), dtype=np.int32)
    osrc = np.full((n, keep_top_k, 2), -1, dtype=np.int32)
    om = np.full((n, keep_top_k), -1, dtype=np.int32)
    for i, cl in enumerate(clusters):
        k = min(len(cl), keep_top_k)
        oc[i] = k
        for j in range(k):
            c, conf, box, first, members = cl[j]
            od[i, j, 0] = F(c)
            od[i, j, 1] = conf
            od[i, j, 2:6] = box
            osrc[i, j] = first
            om[i, j] = members
    return od, oc, osrc, om


def fuse_views(dets, count, views, weight, n, thresh=0.55, score_thresh=0.0, keep_top_k=100, stats=None):
    """The whole call.  stats (a list, optional) receives one dict per image."""
    cl = []
    for i in range(n):
        st = {} if stats is not None else None
        cl.append(fuse_image(dets, count, views, weight, i, thresh, score_thresh, st))
        if stats is not None:
            stats.append(st)
    return padded(cl, keep_top_k)


def run(c, stats=None, **kw):
    params = dict(c['kw'])
    params.update(kw)
    return fuse_views(c['dets'], c['count'], c['views'], c['weight'], c['n'], stats=stats, **params)


# ---- the view plan of ppyolo_hip/tta.py, restated --------------------------------------------------------------------------------

def tta_views(sizes, scales, hflip):
    """[(h, w)] -> [(image, scale index, flipped, mirror_w)], scale-major, then image, then plain before flipped."""
    return [(i, si, f, w if f else 0) for si in range(len(scales)) for i, (h, w) in enumerate(sizes) for f in ((0, 1) if hflip else (0,))]


# ---- the shared cases ------------------------------------------------------------------------------------------------------------
# A case is a dict: dets [V, K, 6], count [V], views [V, 4], weight [V], n, and `kw` = the call's parameters.

def case(rows_per_view, views, n, weight=None, K=None, count=None, **kw):
    """rows_per_view: per view a list of (class, score, x0, y0, x1, y1); rows behind a view's list are filled with a row that
    would be admitted, so that a kernel reading past count shows."""
    V = len(rows_per_view)
    K = max(1, max(len(r) for r in rows_per_view)) if K is None else K
    dets = np.zeros((V, K, 6), dtype=F)
    for v in range(V):
        for r in range(K):
            dets[v, r] = (0, 0.99, 5000 + 40 * v, 5000 + 40 * r, 5030 + 40 * v, 5030 + 40 * r)
        for r, row in enumerate(rows_per_view[v]):
            dets[v, r] = row
    cnt = np.array([len(r) for r in rows_per_view] if count is None else count, dtype=np.int32)
    params = dict(thresh=0.55, score_thresh=0.0, keep_top_k=8)
    params.update(kw)
    return dict(dets=dets, count=cnt, views=np.array(views, dtype=np.int32).reshape(V, 4),
                weight=np.ones((V,), dtype=F) if weight is None else np.array(weight, dtype=F), n=n, kw=params)


NAN, INF = float('nan'), float('inf')
PLAIN2 = [(0, 0, 0, 0), (0, 0, 0, 0)]


def hand_cases():
    c = {}
    c['equal_boxes'] = case([[(1, .8, 10, 10, 50, 50)], [(1, .6, 10, 10, 50, 50)]], PLAIN2, 1)
    c['singleton_of_two_views'] = case([[(1, .8, 10, 10, 50, 50)], []], PLAIN2, 1)
    c['weighted_mean'] = case([[(0, .9, 0, 0, 10, 10)], [(0, .3, 2, 0, 12, 10)]], PLAIN2, 1)
    # A and B fuse to (0, 0, 13, 13); C meets that box and neither A nor B; D meets A and not the box the three fused to
    c['fused_not_members'] = case([[(0, .8, 0, 0, 10, 16), (0, .5, 3, 3, 13, 13)], [(0, .8, 0, 0, 16, 10), (0, .4, 0, 6, 10, 16)]],
                                  PLAIN2, 1, thresh=0.4)
    c['iou_equal_to_thresh'] = case([[(0, .9, 0, 0, 3, 1)], [(0, .8, 1, 0, 4, 1)]], PLAIN2, 1, thresh=0.5)
    c['tie_goes_to_the_earlier'] = case([[(0, .9, 0, 0, 10, 10), (0, .8, 4, 0, 14, 10)], [(0, .7, 2, 0, 12, 10)]], PLAIN2, 1)
    c['one_view_three_rows'] = case([[(0, .9, 0, 0, 10, 10), (0, .6, 1, 0, 11, 10), (0, .3, 0, 1, 10, 11)]], [(0, 0, 0, 0)], 1)
    c['two_classes'] = case([[(1, .9, 10, 10, 50, 50), (2, .8, 10, 10, 50, 50)]], [(0, 3, 4, 0)], 1)
    c['view_weight_two'] = case([[(0, .4, 0, 0, 10, 10)], [(0, .6, 2, 0, 12, 10)]], PLAIN2, 1, weight=[2, 1])
    c['mirror'] = case([[(0, .9, 10, 5, 30, 20)]], [(0, 7, 9, 100)], 1)
    # the flipped view sees the object of the plain view mirrored: the two rows are one cluster
    c['mirror_joins'] = case([[(0, .9, 70, 5, 90, 20)], [(0, .7, 10, 5, 30, 20)]], [(0, 0, 0, 0), (0, 0, 0, 100)], 1)
    # left out: a NaN, an inf, a negative class, class 2^24, a score below the threshold, the row at r == count, score 0 and
    # below 0 (score_thresh = -1 lets them pass merge_views' rule), x1 == x0, y1 < y0, x1 < x0 in a mirrored view
    c['left_out'] = case([[(0, .9, 0, 0, 10, 10), (0, .8, 20, NAN, 30, 10), (0, .7, 100, 0, 110, 10)],
                          [(0, INF, 200, 0, 210, 10), (-1, .8, 220, 0, 230, 10), (16777216.0, .8, 240, 0, 250, 10)],
                          [(0, 0.0, 300, 0, 310, 10), (16777215.0, .6, 320, 0, 330, 10), (0, -.5, 340, 0, 350, 10)],
                          [(0, .5, 400, 0, 400, 10), (0, .5, 420, 10, 430, 5), (0, .55, 440, 0, 450, 10)],
                          [(0, .5, 30, 0, 20, 10), (0, .45, 500, 0, 510, 10), (0, .2, 600, 0, 610, 10)]],
                         [(0, 0, 0, 0)] * 4 + [(0, 0, 0, 1000)], 1, count=[2, 3, 5, 3, 3], score_thresh=-1.0)
    c['score_thresh'] = case([[(0, .5, 0, 0, 10, 10), (0, .29, 20, 0, 30, 10), (0, .3, 40, 0, 50, 10)]], [(0, 0, 0, 0)], 1,
                             score_thresh=0.3)
    c['padding_view'] = case([[(0, .5, 0, 0, 10, 10)], [(0, .9, 0, 0, 10, 10)], [(0, .6, 0, 0, 10, 10)]],
                             [(0, 0, 0, 0), (-1, 0, 0, -5), (0, 0, 0, 0)], 1, weight=[1, NAN, 1])
    # equal conf: class ascending, then creation order (all four s tie: created in (view, row) order)
    c['order_on_equal_conf'] = case([[(2, .5, 0, 0, 10, 10), (1, .5, 20, 0, 30, 10), (1, .5, 40, 0, 50, 10), (0, .25, 60, 0, 70, 10)],
                                     [(0, .25, 60, 0, 70, 10)]], PLAIN2, 1)
    c['cut'] = case([[(0, .5 + .01 * i, 20 * i, 0, 20 * i + 10, 10) for i in range(3)], [(0, .7 + .01 * i, 20 * i, 0, 20 * i + 10, 10) for i in range(2)]],
                    [(0, 0, 0, 0), (0, 100, 0, 0)], 1, keep_top_k=3)
    # image 1 of three has no view at all; image 2's only view is listed before image 0's
    c['image_without_view'] = case([[(0, .9, 0, 0, 10, 10)], [(0, .8, 0, 0, 10, 10)], [(0, .6, 1, 0, 11, 10)]],
                                   [(2, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)], 3)
    c['no_rows'] = case([[], []], PLAIN2, 1)
    c['one_row'] = case([[], [(3, .4, 1, 2, 3, 4)]], PLAIN2, 1)
    return c


def from_merge_case(c, thresh, keep_top_k=1024, score_thresh=0.3, mirror=True, pad_every=0, weights=True):
    """A case of tile_merge_ref (views [V, 3]) as a fusion case: every second view is mirrored (its rows are stored mirrored in a
    view 4000 wide, so that they land where they were), the weights cycle through 1, 1.5, 0.5, and, with pad_every, every
    pad_every-th view becomes a padding view (with the best scores, a bad weight and a negative mirror width)."""
    dets = np.array(c['dets'], dtype=F)
    V = dets.shape[0]
    views = np.concatenate([np.asarray(c['views'], dtype=np.int32), np.zeros((V, 1), dtype=np.int32)], axis=1)
    weight = np.array([(1.0, 1.5, 0.5)[v % 3] if weights else 1.0 for v in range(V)], dtype=F)
    for v in range(V):
        if mirror and v % 2 == 1:
            W = 4000
            x0, x1 = dets[v, :, 2].copy(), dets[v, :, 4].copy()
            dets[v, :, 2], dets[v, :, 4] = (F(W) - x1).astype(F), (F(W) - x0).astype(F)
            views[v, 3] = W
        if pad_every and v % pad_every == pad_every - 1:
            views[v] = (-1, 0, 0, -7)
            weight[v] = NAN
            dets[v, :, 1] = F(0.999)
    return dict(dets=dets, count=np.array(c['count'], dtype=np.int32), views=views, weight=weight, n=c['n'],
                kw=dict(thresh=thresh, score_thresh=score_thresh, keep_top_k=keep_top_k))


SPREAD_V = (1, 2, 6, 41)
SEEDS = (0, 1, 2, 3)


def spread_case(seed, V, K=100, **kw):
    """The clustered recipe of tile_merge_ref dealt to V views, mirrors on half of them."""
    return from_merge_case(T.spread_case(seed, V, K), 0.55, **kw)


# admitted rows per image at the kernel's stage boundaries: a 64-row chunk of a wave's walk, the counting sort's 1024, the stage
BOUNDARIES = T.BOUNDARIES


def uniform_case(R, V, K, thresh=0.3, **kw):
    return from_merge_case(T.uniform_case(R, V, K), thresh, **kw)


MANY_VIEWS = ((63, 3), (64, 3), (65, 3), (130, 5))      # (V, K), every fourth view a padding view


def many_views_case(V, K):
    return spread_case(V % 4, V, K, pad_every=4)


def one_class_case(rows=2048, V=16, K=128, **kw):
    """rows = V * K rows, all of class 0: one segment, walked by one wave."""
    c = T.uniform_case(rows, V, K)
    c['dets'][:, :, 0] = 0
    return from_merge_case(c, 0.3, **kw)


def many_classes_case():
    """The clustered recipe over 80 classes."""
    c = T.spread_case(1, 7, 100)
    r = np.random.RandomState(5)
    c['dets'][:, :, 0] = r.randint(0, 80, size=c['dets'].shape[:2])
    return from_merge_case(c, 0.45)


def poisoned_case():
    """Image 0: a view full of NaN beside a clean view; image 1: clean.  The clean images' results are those they have alone."""
    a, b = spread_case(0, 2, 100), spread_case(1, 2, 100)
    dets = np.concatenate([a['dets'], b['dets']])
    dets[1, ::2, 2:6] = NAN
    dets[1, 1::2, 1] = NAN
    views = np.concatenate([a['views'], b['views']])
    views[2:, 0] = 1
    return dict(dets=dets, count=np.concatenate([a['count'], b['count']]), views=views, weight=np.concatenate([a['weight'], b['weight']]),
                n=2, kw=dict(a['kw']))
