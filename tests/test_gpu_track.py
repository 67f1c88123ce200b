"""ppy_track_update_f32 (csrc/track.hip) through ppyolo_hip.track.Tracker against the float32 numpy restatement tests/track_ref.py,
byte for byte: rows, count, ids, src, hits AND Tracker.state() after every frame.  The cases are the restatement's own
(tests/test_track_ref.py derives the hand cases' answers and checks on the CPU that the float64 run makes the same matches on every
one of them)."""
import functools

import numpy as np
import pytest
import torch

import track_ref as R

pytestmark = pytest.mark.gpu
NAMES = ('rows', 'count', 'ids', 'src', 'hits', 'state')


@functools.lru_cache(None)
def cases():
    return R.fixtures()


@functools.lru_cache(None)
def want(name):
    return R.run_case(cases()[name])


def gpu_run(c):
    """The kernel on a case -> per frame (rows, count, ids, src, hits, state) as numpy."""
    from ppyolo_hip.track import Tracker
    tr = Tracker(c.get('streams', 1), 'cuda', **c['kw'])
    out = []
    for fi, (dets, count) in enumerate(c['frames']):
        for f, s in c.get('resets', ()):
            if f == fi:
                tr.reset([s])
        res = tr.update(torch.from_numpy(np.ascontiguousarray(dets)).cuda(), torch.from_numpy(np.ascontiguousarray(count)).cuda())
        out.append(tuple(t.cpu().numpy() for t in res) + (tr.state(),))
    return out


def same(got, ref, what=''):
    assert len(got) == len(ref)
    for fi, (g, w) in enumerate(zip(got, ref)):
        for a, b, name in zip(g, w[:6], NAMES):
            assert a.dtype == b.dtype and a.shape == b.shape, (what, fi, name, a.dtype, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), (what, fi, name, np.argwhere(a.view(np.int32) != b.view(np.int32))[:4])


def check(name):
    got = gpu_run(cases()[name])
    same(got, want(name)[0], name)
    return got


def test_synthetic_scene_of_12_objects_over_40_frames():
    got = check('synthetic')
    counts = [int(g[1][0]) for g in got]
    assert len(got) == 40 and min(counts) < 12 <= max(counts)
    assert got[-1][5][0, 0] == 40 and got[-1][5][0, 1] > 12          # the kernel's frame counter; clutter took ids too


def test_empty_frames_and_streams_without_a_frame_in_a_batch_of_3():
    c = cases()['batch']
    got = check('batch')
    assert not got[0][5][2].any() and got[0][1][2] == 0 and (got[0][0][2] == -1).all()      # count = -1: untouched, nothing out
    assert got[3][1][1] == 0 and got[3][5][1, 0] == 4                                       # count = 0: a frame with no rows
    for i in range(3):                                                                       # each stream is what it is alone
        one = gpu_run(R.alone(c, i))
        for a, b in zip(got, one):
            for k in range(6):
                assert a[k][i].tobytes() == b[k][0].tobytes(), (i, NAMES[k])


@pytest.mark.parametrize('name', ['one_slot_one_row', 'slots_11_of_12', 'slots_13_of_12'])
def test_fewer_slots_than_objects_counts_the_dropped(name):
    got = check(name)
    dropped = int(got[-1][5][0, 2])
    assert (dropped == 0) == (name == 'slots_13_of_12')


@pytest.mark.parametrize('edge', R.CHUNK_EDGES)
def test_rows_and_slots_at_the_lane_group_edges(edge):
    """Both sides of every size at which the rows (or the slots) get fewer lanes each, a wave's 64 included, and the most of both."""
    got = check('chunk_%d_%d_%d' % edge)
    objects, K, T = edge
    assert int(got[-1][1][0]) == min(objects, K, T)


def test_nan_inf_flat_rows_and_scores_exactly_at_the_thresholds():
    got = check('edge_rows')
    assert got[1][2][0, :4].tolist() == [2, 3, 4, 5] and got[2][2][0, :6].tolist() == [1, 2, 3, 4, 5, 6]
    assert np.isfinite(got[1][0][0, :4]).all()


@pytest.mark.parametrize('name', ['ties', 'ties_agnostic'])
def test_exact_ties_duplicate_rows_and_two_tracks_on_one_box(name):
    got = check(name)
    assert got[1][2][0, :3].tolist() == [1, 2, 3] and got[1][3][0, :3].tolist() == [1, 0, 3]


def test_chain_that_settles_one_pair_a_round():
    got = check('chain')
    assert want('chain')[1][0].stats[1][0] == 16
    assert got[1][2][0].tolist() == list(range(1, 17)) and got[1][3][0].tolist() == list(range(16))


@pytest.mark.parametrize('name', ['crowd_130', 'crowd_600'])
def test_crowd_where_every_stage_takes_several_rounds(name):
    """Dense overlaps: several tracks above the threshold for every row, in every lane group, low rows and new tracks among them."""
    check(name)
    rounds = np.array(want(name)[1][0].stats)
    assert rounds[:, 0].max() >= 3 and rounds[:, 1].max() >= 1 and rounds[:, 2].max() >= 1


def test_class_agnostic_0_and_1_differ():
    a, b = check('class_0'), check('class_1')
    assert [int(g[1][0]) for g in a] == [1, 0, 1] and a[2][2][0, 0] == 2
    assert [int(g[1][0]) for g in b] == [1, 1, 1] and b[2][2][0, 0] == 1


def test_max_lost_0_frees_a_track_the_frame_it_is_lost():
    got = check('max_lost_0')
    assert got[-1][5][0, :3].tolist() == [6, 2, 0]


def test_reset_of_one_stream_in_the_middle():
    got = check('reset')
    assert got[6][5][1, 0] == 1 and got[6][5][0, 0] == 7


def test_two_runs_give_the_same_bytes():
    for name in ('synthetic', 'chunk_513_512_513'):
        a, b = gpu_run(cases()[name]), gpu_run(cases()[name])
        for x, y in zip(a, b):
            for k in range(6):
                assert x[k].tobytes() == y[k].tobytes()


def test_reset_all_and_stale_outputs():
    """reset() of every stream gives a fresh tracker; the state of a fresh tracker is all zero."""
    from ppyolo_hip.track import Tracker
    c = cases()['ties']
    tr = Tracker(1, 'cuda', **c['kw'])
    assert not tr.state().any()
    for _ in range(2):
        for fi, (dets, count) in enumerate(c['frames']):
            res = tr.update(torch.from_numpy(dets).cuda(), torch.from_numpy(count).cuda())
            for a, b in zip(res, want('ties')[0][fi][:5]):
                assert a.cpu().numpy().tobytes() == b.tobytes()
        tr.reset()
        assert not tr.state().any()


def test_update_refuses_what_does_not_fit():
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.track import Tracker
    tr = Tracker(2, 'cuda', max_tracks=4)
    count = torch.zeros(2, dtype=torch.int32, device='cuda')
    with pytest.raises(PPYoloHipError, match='K = 1025 rows per frame, supported: 1..1024'):
        tr.update(torch.zeros((2, 1025, 6), device='cuda'), count)
    with pytest.raises(PPYoloHipError, match='dets has 3 streams, the tracker 2'):
        tr.update(torch.zeros((3, 10, 6), device='cuda'), count)
    with pytest.raises(PPYoloHipError, match=r'count: expected an int32 tensor \[2\]'):
        tr.update(torch.zeros((2, 10, 6), device='cuda'), count.long())
    with pytest.raises(PPYoloHipError, match='stream 2: the tracker has streams 0..1'):
        tr.reset([2])
    assert not tr.state().any()


def test_captured_update_replayed_for_5_frames():
    """One update captured on a single stream and replayed by refilling its static inputs: the frame counter is the kernel's and
    nothing is read on the host, so the replays are the eager frames."""
    from ppyolo_hip.track import Tracker
    c = cases()['graph']
    ref = want('graph')[0]
    frames = c['frames']
    tr = Tracker(1, 'cuda', **c['kw'])
    dets, count = torch.from_numpy(frames[0][0]).cuda(), torch.from_numpy(frames[0][1]).cuda()
    res = tr.update(dets, count)                       # frame 1, eager (it also raises the kernel's LDS limit outside the capture)
    same([tuple(t.cpu().numpy() for t in res) + (tr.state(),)], ref[:1], 'eager')
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = tr.update(dets, count)
    got = []
    for d, n in frames[1:]:
        dets.copy_(torch.from_numpy(d))
        count.copy_(torch.from_numpy(n))
        g.replay()
        torch.cuda.synchronize()
        got.append(tuple(t.cpu().numpy() for t in out) + (tr.state(),))
    assert len(got) == 5
    same(got, ref[1:], 'replay')
    eager = gpu_run(c)
    same(eager, ref, 'eager run')
