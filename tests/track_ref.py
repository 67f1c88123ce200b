"""Sequential numpy restatement of the tracker (csrc/track.hip; include/ppyolo_hip.h has the contract), and the scenes shared by
tests/test_track_ref.py (hand-worked answers, float32 against float64) and tests/test_gpu_track.py (bit-for-bit comparison).

Every scalar is of ONE dtype F (np.float32 by default, so each operation rounds once to float32 as the kernel does; TrackRef(...,
dtype=np.float64) runs the same code in float64).  The thresholds and the constants are float32 values in both runs, as they are
in ppy_track_params_t and in the kernel; the rows are float32 input in both.

    state    per stream a header (frame, ids issued, dropped) and max_tracks slots: state, id, class, score, hits, last and four
             filters (cx, cy, a = w / h, h) of (x, v, Ppp, Ppv, Pvv) each
    predict  every slot that is not FREE; associate in three greedy stages; update; demote and free; open; output by id
"""
import numpy as np

FREE, NEW, TRACKED, LOST = 0, 1, 2, 3
SLOT_WORDS, HEAD_WORDS = 28, 4          # the state buffer's layout, 32-bit words
CX, CY, A, H = 0, 1, 2, 3
X, V, PPP, PPV, PVV = 0, 1, 2, 3, 4


def iou_matrix(tb, rb):
    """tb [T, 4] predicted boxes, rb [R, 4] row boxes, one dtype -> [T, R]: JaccardOverlap(a = the row, b = the track) with
    norm = 0, as PPY_MERGE_IOU: 0 for disjoint boxes, the area of a box with x1 < x0 or y1 < y0 is 0."""
    F = tb.dtype.type
    a = rb[None, :, :]
    b = tb[:, None, :]
    with np.errstate(all='ignore'):
        disjoint = (b[..., 0] > a[..., 2]) | (b[..., 2] < a[..., 0]) | (b[..., 1] > a[..., 3]) | (b[..., 3] < a[..., 1])
        iw = np.where(b[..., 2] < a[..., 2], b[..., 2], a[..., 2]) - np.where(a[..., 0] < b[..., 0], b[..., 0], a[..., 0])
        ih = np.where(b[..., 3] < a[..., 3], b[..., 3], a[..., 3]) - np.where(a[..., 1] < b[..., 1], b[..., 1], a[..., 1])
        inter = iw * ih

        def area(x):
            return np.where((x[..., 2] < x[..., 0]) | (x[..., 3] < x[..., 1]), F(0), (x[..., 2] - x[..., 0]) * (x[..., 3] - x[..., 1]))
        m = inter / ((area(a) + area(b)) - inter)
        return np.where(disjoint, F(0), m).astype(tb.dtype)


def pairs_of(m, thr, tids, tcls, rcls, tsel, rsel, class_agnostic):
    """The pairs a stage considers: (slot t in tsel, row r in rsel) with m[t, r] > thr (a NaN is not), of equal classes unless
    class_agnostic -> [(-IoU, track id, row, slot)]."""
    tsel, rsel = np.asarray(tsel, dtype=np.int64), np.asarray(rsel, dtype=np.int64)
    if not len(tsel) or not len(rsel):
        return []
    sub = m[np.ix_(tsel, rsel)]
    with np.errstate(invalid='ignore'):
        ok = sub > thr
    if not class_agnostic:
        ok &= tcls[tsel][:, None] == rcls[rsel][None, :]
    return [(-float(sub[i, j]), int(tids[tsel[i]]), int(rsel[j]), int(tsel[i])) for i, j in np.argwhere(ok)]


def greedy(pairs):
    """The contract's rule: the pairs in the order IoU descending, track id ascending, row ascending; a pair is taken iff both
    ends are still free -> {slot: row}."""
    got, used = {}, set()
    for _, _, r, t in sorted(pairs):
        if t not in got and r not in used:
            got[t] = r
            used.add(r)
    return got


def mutual_best(pairs):
    """The same matching the way the kernel reaches it: rounds in which every free row names its best free track (IoU, then id)
    and every free track its best free row (IoU, then row); the pairs that name each other are taken.  -> ({slot: row}, the
    rounds that took a pair)."""
    got, used, rounds = {}, set(), 0
    while True:
        pairs = [p for p in pairs if p[3] not in got and p[2] not in used]
        rbest, tbest = {}, {}
        for p in pairs:
            if p[2] not in rbest or p[:2] < rbest[p[2]][:2]:
                rbest[p[2]] = p
            if p[3] not in tbest or (p[0], p[2]) < (tbest[p[3]][0], tbest[p[3]][2]):
                tbest[p[3]] = p
        new = [(t, p[2]) for t, p in tbest.items() if rbest[p[2]][3] == t]
        if not new:
            return got, rounds
        rounds += 1
        for t, r in new:
            got[t] = r
            used.add(r)


class TrackRef(object):
    """One stream's tracker.  update(dets [K, 6] float32, count) -> (rows float32 [max_tracks, 6], count, ids, src, hits) with -1
    padding; `boxes` of the last call keeps the posterior boxes in the run's own dtype."""

    def __init__(self, max_tracks=256, high_thresh=0.6, low_thresh=0.1, new_thresh=None, match_thresh=(0.2, 0.5, 0.3), max_lost=30,
                 class_agnostic=False, dtype=np.float32):
        self.F = F = dtype
        self.T = int(max_tracks)
        f32 = np.float32
        self.high, self.low = F(f32(high_thresh)), F(f32(low_thresh))
        self.new = F(f32(high_thresh + 0.1 if new_thresh is None else new_thresh))
        self.match = [F(f32(v)) for v in match_thresh]
        self.max_lost, self.agnostic = int(max_lost), bool(class_agnostic)
        self.c_apos, self.c_avel, self.c_ameas = F(f32(1e-4)), F(f32(1e-10)), F(f32(1e-2))
        self.stats = []                 # per call: the rounds a mutual-best kernel needs in the three stages
        self.reset()

    def reset(self):
        T = self.T
        self.frame = self.issued = self.dropped = 0
        self.st = np.zeros(T, np.int32)
        self.id = np.zeros(T, np.int32)
        self.cls = np.zeros(T, np.int32)
        self.score = np.zeros(T, np.float32)
        self.hits = np.zeros(T, np.int32)
        self.last = np.zeros(T, np.int32)
        self.f = np.zeros((T, 4, 5), self.F)
        self.matches, self.boxes = {}, np.zeros((0, 4), self.F)

    def box(self, t):
        F, f = self.F, self.f[t]
        with np.errstate(all='ignore'):
            w = F(f[A, X] * f[H, X])
            hw, hh = F(w * F(0.5)), F(f[H, X] * F(0.5))
            return np.array([F(f[CX, X] - hw), F(f[CY, X] - hh), F(f[CX, X] + hw), F(f[CY, X] + hh)], dtype=F)

    def _predict(self, t):
        F, f = self.F, self.f[t]
        with np.errstate(all='ignore'):
            if self.st[t] != TRACKED:
                f[H, V] = F(0)
            h = f[H, X]
            tp, tv = F(h / F(20)), F(h / F(160))
            qp, qv = F(tp * tp), F(tv * tv)
            for k in range(4):
                x, v, ppp, ppv, pvv = f[k]
                p, q = (self.c_apos, self.c_avel) if k == A else (qp, qv)
                f[k, X] = F(x + v)
                f[k, PPP] = F(F(F(ppp + ppv) + F(ppv + pvv)) + p)
                f[k, PPV] = F(ppv + pvv)
                f[k, PVV] = F(pvv + q)

    @staticmethod
    def measure(F, b):
        """the row's box (float32) -> z = (cx, cy, w / h, h) in F"""
        with np.errstate(all='ignore'):
            x0, y0, x1, y1 = (F(v) for v in b)
            w, h = F(x1 - x0), F(y1 - y0)
            return F(x0 + F(w * F(0.5))), F(y0 + F(h * F(0.5))), F(w / h), h

    def _update(self, t, z):
        F, f = self.F, self.f[t]
        with np.errstate(all='ignore'):
            tr = F(f[H, X] / F(20))
            rp = F(tr * tr)
            for k in range(4):
                x, v, ppp, ppv, pvv = f[k]
                s = F(ppp + (self.c_ameas if k == A else rp))
                kp, kv = F(ppp / s), F(ppv / s)
                y = F(z[k] - x)
                f[k, X] = F(x + F(kp * y))
                f[k, V] = F(v + F(kv * y))
                f[k, PPP] = F(ppp - F(kp * ppp))
                f[k, PPV] = F(ppv - F(kp * ppv))
                f[k, PVV] = F(pvv - F(kv * ppv))

    def _open(self, t, z):
        F, f = self.F, self.f[t]
        with np.errstate(all='ignore'):
            h = z[H]
            tp, tv = F(F(F(2) * h) / F(20)), F(F(F(10) * h) / F(160))
            for k in range(4):
                f[k] = (z[k], F(0), self.c_apos if k == A else F(tp * tp), F(0), self.c_avel if k == A else F(tv * tv))

    def update(self, dets, count):
        F, T = self.F, self.T
        dets = np.asarray(dets, dtype=np.float32)
        K = dets.shape[0]
        out = (np.full((T, 6), -1, np.float32), 0, np.full(T, -1, np.int32), np.full(T, -1, np.int32), np.full(T, -1, np.int32))
        self.boxes = np.zeros((0, 4), F)
        if count < 0:
            self.matches = {}
            return out
        self.frame += 1
        for t in range(T):
            if self.st[t] != FREE:
                self._predict(t)
        pbox = np.stack([self.box(t) for t in range(T)]) if T else np.zeros((0, 4), F)
        # admission
        flag = np.zeros(K, np.int32)            # 0 = not admitted, 1 = low, 2 = high
        rcls = np.zeros(K, np.int32)
        with np.errstate(all='ignore'):
            for r in range(max(0, min(int(count), K))):
                row = dets[r]
                if not np.all(np.isfinite(row)):
                    continue
                if not (row[0] >= 0 and row[0] < np.float32(16777216.0) and row[4] > row[2] and row[5] > row[3]):
                    continue
                if not F(row[1]) >= self.low:
                    continue
                flag[r] = 2 if F(row[1]) >= self.high else 1
                rcls[r] = int(row[0])
        m = iou_matrix(pbox, dets[:, 2:6].astype(F))
        state0 = self.st.copy()
        tmatch, rused = {}, set()
        stat = []
        for stage in range(3):
            if stage == 0:
                tsel = [t for t in range(T) if state0[t] in (TRACKED, LOST)]
                rsel = [r for r in range(K) if flag[r] == 2]
            elif stage == 1:
                tsel = [t for t in range(T) if state0[t] == TRACKED and t not in tmatch]
                rsel = [r for r in range(K) if flag[r] == 1]
            else:
                tsel = [t for t in range(T) if state0[t] == NEW]
                rsel = [r for r in range(K) if flag[r] == 2 and r not in rused]
            pairs = pairs_of(m, self.match[stage], self.id, self.cls, rcls, tsel, rsel, self.agnostic)
            got = greedy(pairs)
            alt, rounds = mutual_best(pairs)
            assert alt == got, 'the mutual-best rounds and the sequential greedy rule disagree'
            stat.append(rounds)
            tmatch.update(got)
            rused.update(got.values())
        self.stats.append(stat)
        self.matches = dict((int(self.id[t]), r) for t, r in tmatch.items())
        # update, demote and free
        src = {}
        for t in range(T):
            if t in tmatch:
                r = tmatch[t]
                self._update(t, self.measure(F, dets[r, 2:6]))
                self.score[t], self.cls[t] = dets[r, 1], rcls[r]
                self.hits[t] += 1
                self.last[t] = self.frame
                self.st[t] = TRACKED
                src[t] = r
            elif self.st[t] == TRACKED:
                self.st[t] = LOST
            elif self.st[t] == NEW:
                self.st[t] = FREE
            if self.st[t] == LOST and self.frame - self.last[t] > self.max_lost:
                self.st[t] = FREE
            if self.st[t] == FREE:
                self._clear(t)
        # open
        for r in range(K):
            if flag[r] == 2 and r not in rused and F(dets[r, 1]) >= self.new:
                free = np.flatnonzero(self.st == FREE)
                if not len(free):
                    self.dropped += 1
                    continue
                t = int(free[0])
                self.issued += 1
                self._open(t, self.measure(F, dets[r, 2:6]))
                self.st[t] = TRACKED if self.frame == 1 else NEW
                self.id[t], self.cls[t], self.score[t], self.hits[t], self.last[t] = self.issued, rcls[r], dets[r, 1], 1, self.frame
                src[t] = r
        # output
        live = sorted((int(self.id[t]), t) for t in src if self.st[t] == TRACKED)
        boxes = []
        for i, (_, t) in enumerate(live):
            b = self.box(t)
            boxes.append(b)
            out[0][i, 0], out[0][i, 1] = np.float32(self.cls[t]), self.score[t]
            with np.errstate(over='ignore'):
                out[0][i, 2:] = b.astype(np.float32)
            out[2][i], out[3][i], out[4][i] = self.id[t], src[t], self.hits[t]
        self.boxes = np.array(boxes, dtype=F).reshape(-1, 4)
        return (out[0], len(live)) + out[2:]

    def _clear(self, t):
        self.st[t] = self.id[t] = self.cls[t] = self.hits[t] = self.last[t] = 0
        self.score[t] = 0
        self.f[t] = 0

    def state_words(self):
        """The stream's state as the kernel keeps it: int32 [4 + 28 max_tracks] (float fields by their bits; float32 runs only)."""
        assert self.F is np.float32
        w = np.zeros((self.T, SLOT_WORDS), np.int32)
        w[:, 0], w[:, 1], w[:, 2], w[:, 4], w[:, 5] = self.st, self.id, self.cls, self.hits, self.last
        w[:, 3] = self.score.view(np.int32)
        w[:, 6:26] = self.f.reshape(self.T, 20).view(np.int32)
        return np.concatenate([np.array([self.frame, self.issued, self.dropped, 0], np.int32), w.reshape(-1)])


def run(frames, streams=1, dtype=np.float32, resets=(), **kw):
    """frames: a list of (dets [n, K, 6], count [n]).  resets: (frame index, stream) pairs reset before that frame.  -> per frame
    (rows [n, T, 6], count [n], ids, src, hits [n, T], state words [n, 4 + 28 T] or None in float64, boxes per stream)."""
    refs = [TrackRef(dtype=dtype, **kw) for _ in range(streams)]
    out = []
    for fi, (dets, count) in enumerate(frames):
        for f, s in resets:
            if f == fi:
                refs[s].reset()
        res = [refs[i].update(dets[i], int(count[i])) for i in range(streams)]
        state = np.stack([r.state_words() for r in refs]) if dtype is np.float32 else None
        out.append((np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32), np.stack([r[2] for r in res]),
                    np.stack([r[3] for r in res]), np.stack([r[4] for r in res]), state, [r.boxes for r in refs],
                    [dict(r.matches) for r in refs]))
    return out, refs


# ---- scenes -----------------------------------------------------------------------------------------------------------------

def rows_of(boxes, K, scores=None, classes=None):
    """[(x0, y0, x1, y1)] -> (dets [K, 6], count) with score 0.9 and class 0 unless given."""
    d = np.zeros((K, 6), np.float32)
    for i, b in enumerate(boxes):
        d[i] = (0 if classes is None else classes[i], 0.9 if scores is None else scores[i]) + tuple(b)
    return d, len(boxes)


def one_stream(frames):
    return [(d[None], np.array([c], np.int32)) for d, c in frames]


def synthetic_scene(seed, objects=12, frames=40, K=100, size=640.0, classes=3, miss=0.1, dip=0.15, clutter=2):
    """Objects that move with a constant velocity plus jitter in a size x size image; a row is missing with probability `miss`,
    has a low score with probability `dip`; `clutter` false positives a frame; the rows of a frame are shuffled."""
    rng = np.random.RandomState(seed)
    pos = rng.uniform(60, size - 60, (objects, 2))
    vel = rng.uniform(-4, 4, (objects, 2))
    wh = rng.uniform(30, 90, (objects, 2))
    cls = rng.randint(0, classes, objects)
    out = []
    for _ in range(frames):
        pos = pos + vel
        rows = []
        for o in range(objects):
            if rng.rand() < miss:
                continue
            c = pos[o] + rng.normal(0, 1.0, 2)
            s = wh[o] * (1 + rng.normal(0, 0.02, 2))
            score = rng.uniform(0.15, 0.5) if rng.rand() < dip else rng.uniform(0.72, 0.98)
            rows.append((cls[o], score, c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2))
        for _ in range(clutter):
            c, s = rng.uniform(0, size, 2), rng.uniform(10, 60, 2)
            rows.append((rng.randint(0, classes), rng.uniform(0.05, 0.95), c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2))
        rng.shuffle(rows)
        d = np.zeros((K, 6), np.float32)
        n = min(len(rows), K)
        if n:
            d[:n] = np.array(rows[:n], np.float32)
        d[n:] = rng.uniform(0, 1, (K - n, 6)).astype(np.float32) * 50      # what lies behind count is never read
        out.append((d, n))
    return out


def grid_scene(objects, frames, K, seed=0, step=70.0, per_row=32):
    """`objects` boxes on a grid that drift slowly: every object is matched every frame; sizes for the kernel's chunk edges."""
    rng = np.random.RandomState(seed)
    base = np.array([(40 + step * (o % per_row), 40 + step * (o // per_row)) for o in range(objects)], np.float64)
    wh = rng.uniform(30, 50, (objects, 2))
    out = []
    for f in range(frames):
        c = base + 1.5 * f + rng.normal(0, 0.5, base.shape)
        order = rng.permutation(objects)
        rows = [(o % 2, 0.75 + 0.2 * rng.rand(), c[o, 0] - wh[o, 0] / 2, c[o, 1] - wh[o, 1] / 2, c[o, 0] + wh[o, 0] / 2, c[o, 1] + wh[o, 1] / 2)
                for o in order]
        d = np.zeros((K, 6), np.float32)
        d[:objects] = np.array(rows, np.float32)
        out.append((d, objects))
    return out


def crowd_scene(objects, frames, K, seed, area=420.0):
    """Many large boxes in a small area, all of one class, jittered and dimmed: every row has several tracks above the thresholds
    and a stage takes several rounds; low rows and new tracks among them."""
    rng = np.random.RandomState(seed)
    c0 = rng.uniform(40, area, (objects, 2))
    wh = rng.uniform(50, 110, (objects, 2))
    vel = rng.uniform(-3, 3, (objects, 2))
    out = []
    for f in range(frames):
        c = c0 + vel * f + rng.normal(0, 1.5, c0.shape)
        seen = [o for o in rng.permutation(objects) if rng.rand() > 0.15]
        rows = [(0, rng.uniform(0.2, 0.55) if rng.rand() < 0.25 else rng.uniform(0.62, 0.99), c[o, 0] - wh[o, 0] / 2, c[o, 1] - wh[o, 1] / 2,
                 c[o, 0] + wh[o, 0] / 2, c[o, 1] + wh[o, 1] / 2) for o in seen][:K]
        d = np.zeros((K, 6), np.float32)
        if rows:
            d[:len(rows)] = np.array(rows, np.float32)
        out.append((d, len(rows)))
    return out


def chain_scene(links=16, K=32, width=100.0):
    """Two frames: `links` tracks open in frame 1; in frame 2 the rows sit BETWEEN them so that the IoUs fall strictly along the
    path row 0 - track 1 - row 1 - track 2 - ...: a mutual-best round can settle one pair only.  Track i + 1 takes row i."""
    gaps = [10.0 + g for g in range(2 * links)]
    xs, x = [], 0.0
    for g in gaps:
        xs.append(x)
        x += g
    rowx, trackx = xs[0::2], xs[1::2]
    f1 = rows_of([(x, 50.0, x + width, 150.0) for x in trackx], K)
    f2 = rows_of([(x, 50.0, x + width, 150.0) for x in rowx], K)
    return [f1, f2]


def edge_rows_scene(K=16):
    """NaN / Inf rows, flat boxes, a class outside 0..2^24, scores exactly at low, high and new (0.1, 0.6, 0.7) and just below."""
    f32 = np.float32
    below = lambda v: float(np.nextafter(f32(v), f32(0)))
    good = [(10, 10, 60, 80), (100, 10, 150, 80), (200, 10, 250, 80), (300, 10, 350, 80), (400, 10, 450, 80), (500, 10, 550, 80)]
    f1 = rows_of(good, K, scores=[0.7, below(0.7), 0.9, 0.9, 0.9, 0.9])
    bad = np.array([(0, 0.9, np.nan, 10, 60, 80), (0, np.inf, 10, 10, 60, 80), (0, 0.9, 10, 10, 10, 80), (0, 0.9, 10, 80, 60, 10),
                    (-1, 0.9, 10, 10, 60, 80), (16777216.0, 0.9, 10, 10, 60, 80), (np.nan, 0.9, 10, 10, 60, 80),
                    (0, 0.9, 10, 10, np.inf, 80)], np.float32)
    d = np.zeros((K, 6), np.float32)
    d[:8] = bad
    live = [(11, 10, 61, 80), (201, 10, 251, 80), (301, 10, 351, 80), (401, 10, 451, 80), (501, 10, 551, 80), (101, 10, 151, 80)]
    d[8:14] = rows_of(live, 6, scores=[below(0.1), 0.1, below(0.6), 0.6, 0.9, 0.7])[0]
    return [f1, (d, 14), rows_of(good, K)]


def tie_scene(K=8):
    """Exact ties: frame 1 opens two tracks on the SAME box (ids 1 and 2) and a third alone; frame 2 has the box twice (rows 1 and
    3): id 1 takes row 1, id 2 row 3; then one row only: id 1 takes it."""
    b, c = (10, 10, 60, 80), (200, 10, 260, 90)
    return [rows_of([b, c, b], K), rows_of([c, b, c, b], K), rows_of([b], K)]


def class_scene(K=8):
    """The detector changes its mind: the second frame's row has another class.  Per class it opens a second track (and the
    first is lost); class-agnostic it stays one track."""
    b = (10, 10, 60, 80)
    return [rows_of([b], K, classes=[1]), rows_of([b], K, classes=[2]), rows_of([b], K, classes=[2])]


def cross_scene(frames=30, K=4):
    """Two objects of different heights that cross on a line."""
    out = []
    for f in range(frames):
        xa, xb = 20.0 + 12 * f, 380.0 - 12 * f
        out.append(rows_of([(xa, 100, xa + 40, 200), (xb, 110, xb + 44, 190)], K))
    return out


def gap_scene(gap, frames_before=3, frames_after=2, K=4):
    """One still object, `gap` empty frames, the object again."""
    b = (50, 50, 100, 150)
    return [rows_of([b], K)] * frames_before + [rows_of([], K)] * gap + [rows_of([b], K)] * frames_after


GPU_SCENES = {
    'synthetic': lambda: dict(frames=one_stream(synthetic_scene(3)), kw=dict(max_tracks=32)),
    'chain': lambda: dict(frames=one_stream(chain_scene()), kw=dict(max_tracks=16)),
    'edge_rows': lambda: dict(frames=one_stream(edge_rows_scene()), kw=dict(max_tracks=8)),
    'ties': lambda: dict(frames=one_stream(tie_scene()), kw=dict(max_tracks=4)),
    'ties_agnostic': lambda: dict(frames=one_stream(tie_scene()), kw=dict(max_tracks=4, class_agnostic=True)),
    'class_0': lambda: dict(frames=one_stream(class_scene()), kw=dict(max_tracks=4)),
    'class_1': lambda: dict(frames=one_stream(class_scene()), kw=dict(max_tracks=4, class_agnostic=True)),
    'one_slot_one_row': lambda: dict(frames=one_stream([(d[:1], min(c, 1)) for d, c in synthetic_scene(5, objects=2, frames=12, K=4, clutter=0)]),
                                     kw=dict(max_tracks=1)),
    'slots_11_of_12': lambda: dict(frames=one_stream(synthetic_scene(7, frames=10, K=20, miss=0.0, dip=0.0, clutter=0)), kw=dict(max_tracks=11)),
    'slots_13_of_12': lambda: dict(frames=one_stream(synthetic_scene(7, frames=10, K=20, miss=0.0, dip=0.0, clutter=0)), kw=dict(max_tracks=13)),
    'crowd_130': lambda: dict(frames=one_stream(crowd_scene(130, 6, 130, 1)), kw=dict(max_tracks=140)),
    'crowd_600': lambda: dict(frames=one_stream(crowd_scene(600, 4, 600, 2, area=900.0)), kw=dict(max_tracks=640, class_agnostic=True)),
    'max_lost_0': lambda: dict(frames=one_stream(gap_scene(1)), kw=dict(max_tracks=2, max_lost=0)),
}
# The kernel deals K rows (or max_tracks slots) to groups of G = 64, 32, ... 1 lanes, the largest with items x G <= 1024: an edge at
# every 1024 / G; and a wave is 64 threads.  (objects, K, max_tracks): both sides of each edge for the rows, then for the slots.
CHUNK_EDGES = [(16, 16, 17), (17, 17, 16), (32, 33, 32), (33, 32, 33), (63, 64, 65), (65, 65, 64), (128, 129, 128), (129, 128, 129),
               (256, 257, 256), (257, 256, 257), (512, 513, 512), (513, 512, 513), (1024, 1024, 1024)]


def chunk_scene(objects, K, max_tracks):
    n = min(objects, K)
    return dict(frames=one_stream(grid_scene(n, 3, K, seed=objects)), kw=dict(max_tracks=max_tracks))


def batch_scene():
    """Three streams in one call: stream 1 has empty frames (count = 0), stream 2 frames without a call (count = -1), the first
    among them: its first frame is the second call."""
    a, b, c = synthetic_scene(11, frames=12), synthetic_scene(12, frames=12), synthetic_scene(13, frames=12)
    frames = []
    for f in range(12):
        count = np.array([a[f][1], 0 if f in (3, 4, 8) else b[f][1], -1 if f in (0, 5, 6) else c[f][1]], np.int32)
        frames.append((np.stack([a[f][0], b[f][0], c[f][0]]), count))
    return dict(frames=frames, streams=3, kw=dict(max_tracks=24))


def alone(case, i):
    """Stream i of a case as a case of its own."""
    return dict(frames=[(d[i:i + 1], c[i:i + 1]) for d, c in case['frames']], streams=1, kw=case['kw'],
                resets=[(f, 0) for f, s in case.get('resets', ()) if s == i])


def reset_scene():
    """Two streams; stream 1 is reset before frame 6: it starts again at frame 1 and id 1, stream 0 goes on."""
    a, b = synthetic_scene(21, frames=10, K=40), synthetic_scene(22, frames=10, K=40)
    return dict(frames=[(np.stack([a[f][0], b[f][0]]), np.array([a[f][1], b[f][1]], np.int32)) for f in range(10)], streams=2,
                kw=dict(max_tracks=24), resets=[(6, 1)])


def graph_scene():
    """Six frames of one stream: the first eager, five replayed from a captured update."""
    return dict(frames=one_stream(synthetic_scene(31, frames=6, K=100)), kw=dict(max_tracks=32))


def fixtures():
    """Every case tests/test_gpu_track.py runs: {name: dict(frames, streams, kw, resets)}."""
    out = {name: make() for name, make in GPU_SCENES.items()}
    for e in CHUNK_EDGES:
        out['chunk_%d_%d_%d' % e] = chunk_scene(*e)
    out.update(batch=batch_scene(), reset=reset_scene(), graph=graph_scene())
    for c in out.values():
        c.setdefault('streams', 1)
        c.setdefault('resets', [])
    return out


def run_case(c, dtype=np.float32):
    return run(c['frames'], streams=c.get('streams', 1), dtype=dtype, resets=c.get('resets', ()), **c['kw'])
