"""Timings of one tracker update (ppyolo_hip/track.py Tracker, csrc/track.hip) for n = 1 and 8 streams, K = 100 rows per frame, with
about 30 and about 200 live tracks per stream, in ONE process with the legs alternating:

  (a) update, device   the launch alone: 20 consecutive updates captured into one graph and replayed, device timestamps (events)
                       around the replays of a window, per update;
  (b) update, eager    Tracker.update called from Python, one frame after the other (five output tensors and one launch a call),
                       host clock over a window that ends in a synchronise;
  (c) host, today      what a user of the parent commit does: copy the rows and counts to the host (which waits for the stream),
                       associate in numpy (HostTracker below: the same tracker, vectorised), one stream after the other; host clock.

The scenes are static boxes on a grid, so every frame does the same work.  30 live tracks: 30 rows a frame, all matched.  200 live
tracks: two sets of 100 boxes take turns frame by frame, so 100 tracks are matched (half of them back from LOST) and 100 are lost
in every frame -- K = 100 caps the rows of a frame, and a track that is live but unseen still costs its prediction and its IoUs.
Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.

    python tools/track_bench.py [--out profiles/track_bench.txt] [--seconds 0.5] [--rounds 5]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import track_ref as R  # noqa: E402

K, REPS = 100, 20


class HostTracker(object):
    """The tracker of include/ppyolo_hip.h on the host, one stream, float32, vectorised over slots and pairs the way a numpy user
    would write it.  update(dets [K, 6], count) -> (ids, rows) of the tracks seen in this frame, by id."""

    def __init__(self, max_tracks=256, high=0.6, low=0.1, new=0.7, match=(0.2, 0.5, 0.3), max_lost=30):
        self.T, self.high, self.low, self.new = max_tracks, np.float32(high), np.float32(low), np.float32(new)
        self.match, self.max_lost = [np.float32(m) for m in match], max_lost
        self.frame = self.issued = self.dropped = 0
        self.st = np.zeros(max_tracks, np.int32)
        self.id, self.cls, self.hits, self.last = (np.zeros(max_tracks, np.int32) for _ in range(4))
        self.score = np.zeros(max_tracks, np.float32)
        self.f = np.zeros((max_tracks, 4, 5), np.float32)

    def boxes(self):
        x = self.f[:, :, 0]
        hw, hh = x[:, 2] * x[:, 3] * np.float32(0.5), x[:, 3] * np.float32(0.5)
        return np.stack([x[:, 0] - hw, x[:, 1] - hh, x[:, 0] + hw, x[:, 1] + hh], axis=1)

    @staticmethod
    def measure(b):
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        return np.stack([b[:, 0] + w * np.float32(0.5), b[:, 1] + h * np.float32(0.5), w / h, h], axis=1)

    def update(self, dets, count):
        if count < 0:
            return np.zeros(0, np.int32), np.zeros((0, 6), np.float32)
        f = self.f
        self.frame += 1
        live = self.st != R.FREE
        f[(self.st != R.TRACKED), 3, 1] = 0
        h = f[:, 3, 0].copy()
        qp, qv = np.repeat(((h / np.float32(20)) ** 2)[:, None], 4, 1), np.repeat(((h / np.float32(160)) ** 2)[:, None], 4, 1)
        qp[:, 2], qv[:, 2] = np.float32(1e-4), np.float32(1e-10)
        x, v, ppp, ppv, pvv = (f[:, :, i].copy() for i in range(5))
        pred = np.stack([x + v, v, ((ppp + ppv) + (ppv + pvv)) + qp, ppv + pvv, pvv + qv], axis=2)
        f[live] = pred[live]
        n = max(0, min(int(count), len(dets)))
        rows = dets[:n]
        with np.errstate(all='ignore'):
            ok = np.isfinite(rows).all(1) & (rows[:, 0] >= 0) & (rows[:, 0] < 16777216.0) & (rows[:, 4] > rows[:, 2]) & \
                (rows[:, 5] > rows[:, 3]) & (rows[:, 1] >= self.low)
            level = np.where(ok, np.where(rows[:, 1] >= self.high, 2, 1), 0)
            rcls = np.where(ok, rows[:, 0], 0).astype(np.int32)
            m = R.iou_matrix(self.boxes(), np.ascontiguousarray(rows[:, 2:6]))
        st0 = self.st.copy()
        tmatch = np.full(self.T, -1, np.int64)
        rmatch = np.full(n, -1, np.int64)
        for stage in range(3):
            tsel = ((st0 == R.TRACKED) | ((st0 == R.LOST) & (stage == 0))) if stage < 2 else (st0 == R.NEW)
            mask = (m > self.match[stage]) & (tsel & (tmatch < 0))[:, None] & ((level == (1 if stage == 1 else 2)) & (rmatch < 0))[None, :] & \
                (self.cls[:, None] == rcls[None, :])
            tt, rr = np.nonzero(mask)
            for i in np.lexsort((rr, self.id[tt], -m[tt, rr])):
                if tmatch[tt[i]] < 0 and rmatch[rr[i]] < 0:
                    tmatch[tt[i]], rmatch[rr[i]] = rr[i], tt[i]
        hit = tmatch >= 0
        if hit.any():
            z = self.measure(rows[tmatch[hit], 2:6])
            g = f[hit]
            r = np.repeat(((g[:, 3, 0] / np.float32(20)) ** 2)[:, None], 4, 1)
            r[:, 2] = np.float32(1e-2)
            x, v, ppp, ppv, pvv = (g[:, :, i] for i in range(5))
            s = ppp + r
            kp, kv, y = ppp / s, ppv / s, z - x
            f[hit] = np.stack([x + kp * y, v + kv * y, ppp - kp * ppp, ppv - kp * ppv, pvv - kv * ppv], axis=2)
            self.score[hit], self.cls[hit] = rows[tmatch[hit], 1], rcls[tmatch[hit]]
            self.hits[hit] += 1
            self.last[hit] = self.frame
        self.st[~hit & (st0 == R.NEW)] = R.FREE
        self.st[~hit & (st0 == R.TRACKED)] = R.LOST
        self.st[hit] = R.TRACKED
        self.st[(self.st == R.LOST) & (self.frame - self.last > self.max_lost)] = R.FREE
        gone = self.st == R.FREE
        for a in (self.id, self.cls, self.hits, self.last, self.score, f):
            a[gone] = 0
        seen = hit.copy()
        want = np.flatnonzero((level == 2) & (rmatch < 0) & (rows[:, 1] >= self.new))
        free = np.flatnonzero(gone)
        k = min(len(want), len(free))
        self.dropped += len(want) - k
        if k:
            t, r = free[:k], want[:k]
            z = self.measure(rows[r, 2:6])
            p = np.repeat((np.float32(2) * z[:, 3] / np.float32(20))[:, None] ** 2, 4, 1)
            q = np.repeat((np.float32(10) * z[:, 3] / np.float32(160))[:, None] ** 2, 4, 1)
            p[:, 2], q[:, 2] = np.float32(1e-4), np.float32(1e-10)
            zero = np.zeros_like(z)
            f[t] = np.stack([z, zero, p, zero, q], axis=2)
            self.st[t] = R.TRACKED if self.frame == 1 else R.NEW
            self.id[t] = self.issued + 1 + np.arange(k)
            self.cls[t], self.score[t], self.hits[t], self.last[t] = rcls[r], rows[r, 1], 1, self.frame
            self.issued += k
            seen[t] = True
        out = np.flatnonzero(seen & (self.st == R.TRACKED))
        out = out[np.argsort(self.id[out])]
        return self.id[out], np.concatenate([self.cls[out, None].astype(np.float32), self.score[out, None], self.boxes()[out]], axis=1)


def grid_rows(objects, seed, offset=0.0):
    """`objects` boxes on a grid -> dets [K, 6]"""
    rng = np.random.RandomState(seed)
    wh = rng.uniform(30, 50, (objects, 2))
    d = np.zeros((K, 6), np.float32)
    for o in range(objects):
        cx, cy = 40 + offset + 70.0 * (o % 16), 40 + 70.0 * (o // 16)
        d[o] = (o % 3, 0.75 + 0.2 * rng.rand(), cx - wh[o, 0] / 2, cy - wh[o, 1] / 2, cx + wh[o, 0] / 2, cy + wh[o, 1] / 2)
    return d


def scene(n, live):
    """-> (the frames of the warm-up, the frames that take turns afterwards), each (dets [n, K, 6], count [n]) numpy"""
    if live <= K:
        a = np.stack([grid_rows(live, 10 + i) for i in range(n)])
        c = np.full(n, live, np.int32)
        return [(a, c)] * 2, [(a, c)]
    half = live // 2
    a = np.stack([grid_rows(half, 10 + i) for i in range(n)])
    b = np.stack([grid_rows(half, 50 + i, offset=35.0 * 16 * 2) for i in range(n)])
    c = np.full(n, half, np.int32)
    return [(a, c), (b, c), (b, c)], [(a, c), (b, c)]      # the second set needs two frames in a row to be confirmed


def window_host(fn, seconds):
    n = 2
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n
        n = max(n + 1, int(n * min(8.0, 1.15 * seconds / max(dt, 1e-6))))


def window_device(fn, seconds):
    """seconds per call of fn by device timestamps: events around the calls of a window of at least `seconds`"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 2
    while True:
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        if dt >= seconds:
            return dt / n
        n = max(n + 1, int(n * min(8.0, 1.15 * seconds / max(dt, 1e-6))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_bench.txt'))
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('track_bench needs the MI355X: a time taken anywhere else says nothing')
    from ppyolo_hip.track import Tracker
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('%s; K = %d rows a frame, max_tracks = 256; windows >= %.1f s, %d rounds, legs alternating; (a) = %d updates a graph' % (
        torch.cuda.get_device_name(0), K, a.seconds, a.rounds, REPS))
    say()
    for n in (1, 8):
        for live in (30, 200):
            warm, turns = scene(n, live)
            d_turns = [(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()) for d, c in turns]
            # the three trackers see the same frames; their ids must agree before anything is timed
            dev, eager = Tracker(n, 'cuda'), Tracker(n, 'cuda')
            host = [HostTracker() for _ in range(n)]
            for d, c in warm + turns * 2:
                td, tc = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
                got = dev.update(td, tc)
                eager.update(td, tc)
                ids = got[2].cpu().numpy()
                for i in range(n):
                    hid, _ = host[i].update(d[i], int(c[i]))
                    assert ids[i, :int(got[1][i])].tolist() == hid.tolist(), 'the host tracker and the kernel disagree'
            state = dev.state()[0, 4:].reshape(-1, 28)
            n_live, n_out = int((state[:, 0] != 0).sum()), int(got[1][0])

            def chain(tr=dev):
                for k in range(REPS):
                    tr.update(*d_turns[k % len(d_turns)])
            chain()                                     # REPS is even: the graph starts where the turns start
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                chain()
            turn = dict(eager=0, host=0)                # every tracker goes through the turns on its own

            def eager_call():
                eager.update(*d_turns[turn['eager'] % len(d_turns)])
                turn['eager'] += 1

            def host_call():
                td, tc = d_turns[turn['host'] % len(d_turns)]
                turn['host'] += 1
                d, c = td.cpu().numpy(), tc.cpu().numpy()            # waits for the stream
                for i in range(n):
                    host[i].update(d[i], int(c[i]))
                torch.cuda.synchronize()
            got = dict(dev=[], eager=[], host=[])
            for fn in (g.replay, eager_call, host_call):
                for _ in range(3):
                    fn()
            for _ in range(a.rounds):
                got['dev'].append(window_device(g.replay, a.seconds) / REPS)
                got['eager'].append(window_host(eager_call, a.seconds))
                got['host'].append(window_host(host_call, a.seconds / 2))
            med = {k: statistics.median(v) for k, v in got.items()}
            say('n = %d streams, %d live tracks a stream (%d reported a frame)' % (n, n_live, n_out))
            for k, name in (('dev', '(a) update, device timestamps'), ('eager', '(b) update, eager call'), ('host', '(c) host, today: copy + numpy + sync')):
                say('  %-40s %10.1f us per frame   (%.1f .. %.1f)' % (name, med[k] * 1e6, min(got[k]) * 1e6, max(got[k]) * 1e6))
            say('  (c) / (a) = %.0fx, (c) / (b) = %.1fx' % (med['host'] / med['dev'], med['host'] / med['eager']))
            say()
            del g
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
