"""The tracker's numpy restatement (tests/track_ref.py) against hand-worked scenes whose expected ids stand here, the sequential
greedy rule against the mutual-best rounds the kernel uses, and the float32 run against the float64 run of the same code on every
case the GPU tests compare bit for bit (tests/test_gpu_track.py): the two must make the same matches, so that the bit-for-bit
comparison pins a tracker and not a rounding accident."""
import numpy as np
import pytest

import track_ref as R


def ids_of(out):
    """per frame the reported (id, row) pairs of stream 0"""
    return [[(int(o[2][0][j]), int(o[3][0][j])) for j in range(int(o[1][0]))] for o in out]


def run1(frames, **kw):
    out, refs = R.run(R.one_stream(frames), **kw)
    return ids_of(out), refs[0], out


def test_two_objects_that_cross_keep_their_ids():
    frames = R.cross_scene()
    ids, ref, _ = run1(frames, max_tracks=4)
    # they meet at frame 15 (both at x = 200): row 0 stays id 1 and row 1 id 2 through the crossing
    assert ids == [[(1, 0), (2, 1)]] * len(frames)
    assert ref.issued == 2 and ref.dropped == 0


def test_object_missing_for_max_lost_frames_comes_back_with_its_id():
    ids, ref, _ = run1(R.gap_scene(5), max_tracks=2, max_lost=5)
    assert ids == [[(1, 0)]] * 3 + [[]] * 5 + [[(1, 0)]] * 2
    assert ref.issued == 1 and ref.hits[0] == 5 and ref.frame == 10


def test_object_missing_one_frame_longer_comes_back_with_a_new_id():
    ids, ref, _ = run1(R.gap_scene(6), max_tracks=2, max_lost=5)
    # freed in frame 9 (9 - 3 > 5); frame 10 opens id 2 as NEW, which is reported from its second frame on
    assert ids == [[(1, 0)]] * 3 + [[]] * 6 + [[], [(2, 0)]]
    assert ref.issued == 2 and ref.st.tolist() == [R.TRACKED, R.FREE]


def test_tracked_object_kept_alive_by_low_score_rows_only():
    b, other = (50, 50, 100, 150), (300, 50, 350, 150)
    frames = [R.rows_of([b], 4)] * 3 + [R.rows_of([other, b], 4, scores=[0.3, 0.3])] * 5 + [R.rows_of([b], 4)]
    ids, ref, out = run1(frames, max_tracks=4)
    # stage 2 keeps id 1 (row 1 in the low frames); the other low row never opens a track
    assert ids == [[(1, 0)]] * 3 + [[(1, 1)]] * 5 + [[(1, 0)]]
    assert ref.issued == 1 and ref.hits[0] == 9
    assert out[4][0][0, 0, 1] == np.float32(0.3)          # the reported score is the row's


def test_one_frame_false_positive_never_gets_an_id_in_the_output():
    b, fp, late = (50, 50, 100, 150), (300, 300, 340, 380), (500, 50, 560, 150)
    frames = [R.rows_of([b], 4)] * 2 + [R.rows_of([b, fp], 4)] + [R.rows_of([b], 4)] * 2 + [R.rows_of([b, late], 4)] * 2
    ids, ref, _ = run1(frames, max_tracks=4)
    # the false positive takes id 2 as NEW in frame 3 and is freed in frame 4; the late object is id 3, reported on its second frame
    assert ids == [[(1, 0)]] * 6 + [[(1, 0), (3, 1)]]
    assert ref.issued == 3 and sorted(ref.id.tolist()) == [0, 0, 1, 3]


def test_slot_overflow_is_counted_in_dropped():
    boxes = [(50, 50, 100, 150), (200, 50, 250, 150), (350, 50, 400, 150)]
    ids, ref, _ = run1([R.rows_of(boxes, 4)] * 4, max_tracks=2)
    assert ids == [[(1, 0), (2, 1)]] * 4
    assert ref.dropped == 4 and ref.issued == 2          # row 2 asks for a slot in every frame


def test_chain_takes_one_round_per_pair():
    c = R.GPU_SCENES['chain']()
    out, refs = R.run_case(c)
    assert ids_of(out)[1] == [(i + 1, i) for i in range(16)]
    assert refs[0].stats[1][0] == 16          # stage 1 of frame 2: sixteen rounds, one pair each


def test_ties_are_broken_by_id_then_row():
    out, refs = R.run_case(R.GPU_SCENES['ties']())
    ids = ids_of(out)
    assert ids[0] == [(1, 0), (2, 1), (3, 2)]          # ids 1 and 3 sit on the same box
    assert ids[1] == [(1, 1), (2, 0), (3, 3)]          # equal IoUs: the smaller id takes the earlier row
    assert ids[2] == [(1, 0)]


def test_class_agnostic_differs_where_the_class_changes():
    per_class, agnostic = ids_of(R.run_case(R.GPU_SCENES['class_0']())[0]), ids_of(R.run_case(R.GPU_SCENES['class_1']())[0])
    assert per_class == [[(1, 0)], [], [(2, 0)]]
    assert agnostic == [[(1, 0)]] * 3


def test_scores_exactly_at_the_thresholds_and_bad_rows():
    out, refs = R.run_case(R.GPU_SCENES['edge_rows']())
    ids = ids_of(out)
    assert ids[0] == [(1, 0), (2, 2), (3, 3), (4, 4), (5, 5)]          # 0.7 opens, the float below does not
    # frame 2: rows 0..7 are not admitted; row 8 (just below low) is not; row 9 (0.1, low) keeps id 2; row 10 (just below high) is
    # low and keeps id 3; rows 11 (0.6) and 12 are high and keep ids 4 and 5; row 13 (0.7, high, on the box never opened) opens id 6
    assert ids[1] == [(2, 9), (3, 10), (4, 11), (5, 12)]
    # frame 3: id 1 comes back from LOST, id 6 is confirmed by row 1
    assert ids[2] == [(1, 0), (2, 2), (3, 3), (4, 4), (5, 5), (6, 1)]


def test_a_stream_in_a_batch_is_what_it_is_alone():
    for make in (R.batch_scene, R.reset_scene):
        c = make()
        c.setdefault('resets', [])
        out, _ = R.run_case(c)
        for i in range(c['streams']):
            one, _ = R.run_case(R.alone(c, i))
            for a, b in zip(out, one):
                for k in range(6):
                    assert a[k][i].tobytes() == b[k][0].tobytes()


@pytest.fixture(scope='module')
def both():
    out = {}
    for name, c in R.fixtures().items():
        out[name] = (c, R.run_case(c)[0], R.run_case(c, dtype=np.float64)[0])
    return out


def test_float32_and_float64_make_the_same_matches_on_every_gpu_case(both):
    worst = (0.0, None)
    for name, (c, f32, f64) in sorted(both.items()):
        for fi, (a, b) in enumerate(zip(f32, f64)):
            assert a[7] == b[7], (name, fi)                                  # the matches of the three stages, {id: row}
            for k in (1, 2, 3, 4):
                assert np.array_equal(a[k], b[k]), (name, fi, k)             # count, ids, src, hits
            assert np.array_equal(a[0][..., :2], b[0][..., :2]), (name, fi)  # class and score
            for ba, bb in zip(a[6], b[6]):
                if len(ba):
                    d = float(np.abs(ba.astype(np.float64) - bb).max())
                    if d > worst[0]:
                        worst = (d, name)
    print('largest |float32 - float64| of a posterior box coordinate: %.3e px (%s)' % worst)
    assert worst[1] is not None


def test_the_cases_exercise_what_they_name(both):
    syn = both['synthetic'][1]
    counts = [int(o[1][0]) for o in syn]
    assert len(syn) == 40 and min(counts) < 12 <= max(counts)              # misses, and every object seen
    hdr = lambda name: both[name][1][-1][5][0][:3].tolist()                # (frame, issued, dropped) after the last frame
    assert hdr('slots_11_of_12')[2] > 0 and hdr('slots_13_of_12')[2] == 0
    assert hdr('one_slot_one_row')[2] > 0
    assert hdr('chunk_17_17_16')[2] == 3 and hdr('chunk_1024_1024_1024') == [3, 1024, 0]
    assert hdr('max_lost_0') == [6, 2, 0]
    for name in ('crowd_130', 'crowd_600'):                               # every stage matches, the first in several rounds
        rounds = np.array(R.run_case(both[name][0])[1][0].stats)
        assert rounds[:, 0].max() >= 3 and rounds[:, 1].max() >= 1 and rounds[:, 2].max() >= 1
    batch = both['batch'][1]
    assert batch[0][5][2].tolist() == [0] * len(batch[0][5][2])            # the stream without a first frame is untouched
    assert batch[1][5][2][0] == 1                                          # and its first frame is frame 1
    assert both['reset'][1][6][5][1][0] == 1 and both['reset'][1][6][5][0][0] == 7
