"""float32 numpy restatement of PaddleDetection's multiclass_nms operator for one image: the oracle of
tests/test_multiclass_nms_ref.py (hand-derived cases) and tests/test_gpu_multiclass_nms.py (bit-for-bit comparison).

    per class c != background_label, ascending:
        candidates: boxes i with scores[i, c] > score_threshold (strict), by (score descending, box index ascending),
        the first nms_top_k of them; greedy scan in that order: i is selected iff iou(box_i, box_k) <= nms_threshold
        for EVERY already selected k of the class (so a NaN IoU suppresses)
    iou(a, b) in float32, one rounding per operation, norm = 0 if normalized else 1:
        0 if b.x1 > a.x2 or b.x2 < a.x1 or b.y1 > a.y2 or b.y2 < a.y1
        iw = (min(a.x2, b.x2) - max(a.x1, b.x1)) + norm, ih likewise, inter = iw * ih
        area(x) = 0 if x.x2 < x.x1 or x.y2 < x.y1 else ((x.x2 - x.x1) + norm) * ((x.y2 - x.y1) + norm)
        inter / ((area(a) + area(b)) - inter)
    across classes: concatenate the selections (class ascending, selection order inside a class); more than keep_top_k:
        the keep_top_k highest scores, ties to the earlier position; rows (label, score, x1, y1, x2, y2) in
        (class ascending, score descending, box index ascending) order, the score unchanged.

Everything stays in np.float32 arrays (numpy rounds each elementwise operation once; nothing here can fuse)."""
import numpy as np

F = np.float32


def area(b, norm):
    """b [..., 4] float32 -> float32 areas."""
    w = (b[..., 2] - b[..., 0]) + norm
    h = (b[..., 3] - b[..., 1]) + norm
    return np.where((b[..., 2] < b[..., 0]) | (b[..., 3] < b[..., 1]), F(0), w * h).astype(F)


def iou(a, b, normalized=True):
    """iou(a, b) of one box a [4] with boxes b [K, 4] (or one box [4]), all float32 -> float32 [K] (or a scalar)."""
    a = np.asarray(a, dtype=F)
    b = np.asarray(b, dtype=F)
    norm = F(0) if normalized else F(1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        disjoint = (b[..., 0] > a[2]) | (b[..., 2] < a[0]) | (b[..., 1] > a[3]) | (b[..., 3] < a[1])
        # std::min(x, y) = y < x ? y : x ; std::max(x, y) = x < y ? y : x
        x2 = np.where(b[..., 2] < a[2], b[..., 2], a[2])
        x1 = np.where(a[0] < b[..., 0], b[..., 0], a[0])
        y2 = np.where(b[..., 3] < a[3], b[..., 3], a[3])
        y1 = np.where(a[1] < b[..., 1], b[..., 1], a[1])
        iw = ((x2 - x1).astype(F) + norm).astype(F)
        ih = ((y2 - y1).astype(F) + norm).astype(F)
        inter = (iw * ih).astype(F)
        union = ((area(a, norm) + area(b, norm)).astype(F) - inter).astype(F)
        out = (inter / union).astype(F)
    return np.where(disjoint, F(0), out).astype(F)


def nms_one_class(boxes, sc, score_threshold, nms_top_k, nms_threshold, normalized, stats=None):
    """Selected box indices of one class, in selection order.  sc [M] float32."""
    thr = F(nms_threshold)
    cand = np.nonzero(sc > F(score_threshold))[0]
    order = cand[np.lexsort((cand, -sc[cand].astype(np.float64)))]      # score descending, box index ascending
    if stats is not None:
        stats['truncated'] += int(order.size > nms_top_k)
    order = order[:nms_top_k]
    kept = []
    kb = np.zeros((order.size, 4), dtype=F)
    for i in order:
        ok = True
        if kept:
            ok = bool(np.all(iou(boxes[i], kb[:len(kept)], normalized) <= thr))      # NaN <= thr is False: suppressed
        if ok:
            kb[len(kept)] = boxes[i]
            kept.append(int(i))
    if stats is not None:
        stats['suppressed'] += int(order.size - len(kept))
    return kept


def multiclass_nms(boxes, scores, score_threshold, nms_top_k, keep_top_k, nms_threshold=0.3, normalized=True, nms_eta=1.0,
                   background_label=-1, stats=None):
    """boxes [M, 4], scores [M, C] -> (dets [K, 6] float32, keep_idx [K] int64 = box * C + class).  K may be 0.
    stats (a dict, optional) receives: truncated = classes cut at nms_top_k, suppressed = candidates the greedy scan
    dropped, selected = selections before the keep_top_k cut."""
    assert nms_eta == 1.0, 'the adaptive threshold is out of scope'
    boxes = np.ascontiguousarray(boxes, dtype=F)
    scores = np.ascontiguousarray(scores, dtype=F)
    M, C = scores.shape
    if stats is not None:
        stats.update(truncated=0, suppressed=0, selected=0)
    sel = []                                                   # (class, box) in concatenation order
    for c in range(C):
        if c == background_label:
            continue
        sel += [(c, i) for i in nms_one_class(boxes, scores[:, c], score_threshold, nms_top_k, nms_threshold, normalized, stats)]
    if stats is not None:
        stats['selected'] = len(sel)
    if len(sel) > keep_top_k:
        s = np.array([scores[i, c] for c, i in sel], dtype=np.float64)
        top = np.lexsort((np.arange(len(sel)), -s))[:keep_top_k]      # score descending, ties to the earlier position
        sel = [sel[t] for t in top]
    sel.sort(key=lambda ci: (ci[0], -float(scores[ci[1], ci[0]]), ci[1]))
    dets = np.zeros((len(sel), 6), dtype=F)
    keep = np.zeros((len(sel),), dtype=np.int64)
    for r, (c, i) in enumerate(sel):
        dets[r, 0] = c
        dets[r, 1] = scores[i, c]
        dets[r, 2:] = boxes[i]
        keep[r] = i * C + c
    return dets, keep


def padded(results, keep_top_k):
    """[(dets, keep)] per image -> (dets [N, keep_top_k, 6] padded with -1, count [N], keep_idx [N, keep_top_k] padded with -1),
    the form the kernels write."""
    N = len(results)
    d = np.full((N, keep_top_k, 6), -1, dtype=F)
    k = np.full((N, keep_top_k), -1, dtype=np.int32)
    cnt = np.zeros((N,), dtype=np.int32)
    for n, (dd, kk) in enumerate(results):
        cnt[n] = dd.shape[0]
        d[n, :dd.shape[0]] = dd
        k[n, :dd.shape[0]] = kk
    return d, cnt, k


# ---- the shared cases (CPU test 1 checks the restatement on them; GPU tests 3-5 run the kernels on them) ----

def chain(n):
    """n boxes [3i, 0, 3i+10, 10], one class, scores falling from 0.9 to 0.1."""
    i = np.arange(n, dtype=np.float64)
    boxes = np.stack([3 * i, 0 * i, 3 * i + 10, 0 * i + 10], axis=1).astype(F)
    scores = np.linspace(0.9, 0.1, n).astype(F).reshape(n, 1)
    return boxes, scores


def clustered(seed, M=200, C=5, centres=12):
    """Test 4's recipe: jittered copies of `centres` centres and sizes, scores uniform^3 with 20 % set to exactly 0.25."""
    r = np.random.RandomState(seed)
    ctr = r.uniform(20, 300, size=(centres, 2))
    size = r.uniform(20, 80, size=(centres, 2))
    which = r.randint(0, centres, size=M)
    c = ctr[which] + r.normal(0, 4, size=(M, 2))
    s = size[which] * r.uniform(0.85, 1.15, size=(M, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], axis=1).astype(F)
    scores = (r.uniform(0, 1, size=(M, C)) ** 3).astype(F)
    scores[r.uniform(0, 1, size=(M, C)) < 0.2] = F(0.25)
    return boxes, scores


CLUSTERED_CFG = dict(score_threshold=0.05, nms_top_k=64, keep_top_k=40, nms_threshold=0.45, normalized=False)
