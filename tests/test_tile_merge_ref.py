"""The tile plan of ppyolo_hip/tiles.py and the numpy restatement of the cross-view merge (tests/tile_merge_ref.py), on cases whose
answers are derived by hand and written out here; the fairness of the seeded cases tests/test_gpu_tile_merge.py runs (every one
selects and suppresses, the four modes differ, the cut cases cut); and the refusals the host can decide without a device."""
import ctypes

import numpy as np
import pytest

import tile_merge_ref as R

F = np.float32


# ---- the tile plan ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('args,expect', R.GRID_VALUES)
def test_tile_origins_worked_values(args, expect):
    from ppyolo_hip import tiles
    L, T, ov = args
    origins, extent = tiles.tile_origins(L, T, ov)
    assert origins == expect
    assert extent == min(L, T)
    assert R.grid_origins(L, T, ov) == (expect, min(L, T))


def test_tile_origins_refusals():
    from ppyolo_hip import tiles
    from ppyolo_hip._lib import PPYoloHipError
    for bad in [(0, 64, .2), (64, 0, .2), (64, 64, 1.0), (64, 64, -0.1), (64, 64, float('nan'))]:
        with pytest.raises(PPYoloHipError):
            tiles.tile_origins(*bad)


@pytest.mark.parametrize('h,w,tile,ov', [(2160, 3840, 608, .2), (427, 640, 192, .2), (480, 640, 192, .2), (64, 64, 64, .2), (65, 64, 64, 0),
                                         (50, 300, 64, .5), (129, 129, 64, 0), (7, 1000, 64, .9), (300, 200, 192, .99)])
@pytest.mark.parametrize('full_view', [True, False])
def test_plan_views_inside_and_covering(h, w, tile, ov, full_view):
    from ppyolo_hip import tiles
    views = tiles.plan_views(h, w, tile, ov, full_view)
    assert views == R.grid_views(h, w, tile, ov, full_view)
    single = h <= tile and w <= tile
    if single:
        assert views == [(0, 0, w, h)]
    tiles_only = views[1:] if (full_view and not single) else views
    if full_view and not single:
        assert views[0] == (0, 0, w, h)
    assert tiles_only == sorted(tiles_only, key=lambda v: (v[1], v[0]))      # row-major: y outer, x inner
    covered = np.zeros((h, w), dtype=bool)
    for ox, oy, vw, vh in views:
        assert 0 <= ox and 0 <= oy and vw >= 1 and vh >= 1 and ox + vw <= w and oy + vh <= h
    for ox, oy, vw, vh in tiles_only:
        assert (vw, vh) == (min(w, tile), min(h, tile))          # full-size, never cut
        covered[oy:oy + vh, ox:ox + vw] = True
    assert covered.all()


def test_plan_views_4k_frame_has_41_views():
    from ppyolo_hip import tiles
    views = tiles.plan_views(2160, 3840, 608, .2, True)
    assert len(views) == 41 and len(tiles.plan_views(2160, 3840, 608, .2, False)) == 40
    # the two COCO-sized fixtures of the detector test (500 x 375 and 640 x 418) at tile 192: 4 x 3 tiles and the whole image
    assert len(tiles.plan_views(375, 500, 192, .2, True)) == 13 and len(tiles.plan_views(418, 640, 192, .2, True)) == 13


# ---- the restatement on hand-derived cases --------------------------------------------------------------------------------------
# name -> per image the (view, row) selections in output order
HAND_ANSWERS = {
    # the whole object (0.9) first; each half lies inside it: inter / smaller = 10000 / 10000 = 1 > 0.5
    'halves_ios': [[(0, 0)]],
    # iou(half, whole) = 10000 / 20000 = 0.5 <= 0.5; the halves touch at x = 200: iw = 0, iou = 0
    'halves_iou': [[(0, 0), (1, 0), (2, 0)]],
    # left (0.9), right (0.8): disjoint interiors, both stay, in score order; the whole (0.7) meets the left half with ios = 1
    'halves_reversed_ios': [[(1, 0), (2, 0)]],
    'equal_scores': [[(0, 0), (0, 1), (2, 0), (2, 1)], [(1, 0)]],
    'signed_zero': [[(0, 0), (0, 1), (1, 0), (0, 2)]],
    'classes_aware': [[(0, 0), (0, 1)]],
    'classes_agnostic': [[(0, 0)]],
    'truncated_class': [[(0, 0), (0, 2)]],
    'left_out': [[(0, 0), (2, 1), (2, 0)]],
    'padding_view': [[(2, 0), (0, 0)]],
    # two copies of a zero-area box: iou = 0 / 0 = NaN suppresses the second; the real box around it: inter 0, iou 0, selected
    'zero_area_iou': [[(0, 0), (0, 2)]],
    # ios of the real box with the selected zero-area box: 0 / min(0, 200) = NaN: suppressed as well
    'zero_area_ios': [[(0, 0)]],
    # thresh 1.0: nothing is suppressed, copies included (iou = 1 <= 1): the admitted rows in (score, view, row) order
    'thresh_one_iou': [[(2, 1), (0, 0), (1, 0), (2, 0), (0, 1)]],
    # five disjoint boxes, scores 0.71, 0.70, 0.52, 0.51, 0.50: the first three
    'cut': [[(1, 1), (1, 0), (0, 2)]],
}


@pytest.mark.parametrize('name', sorted(HAND_ANSWERS))
def test_hand_cases(name):
    c = R.hand_cases()[name]
    dets, count, src = R.run(c)
    K = c['kw']['keep_top_k']
    expect = HAND_ANSWERS[name]
    assert dets.shape == (c['n'], K, 6) and dets.dtype == F and src.shape == (c['n'], K, 2)
    assert count.tolist() == [len(e) for e in expect]
    for i, e in enumerate(expect):
        assert [tuple(s) for s in src[i, :len(e)].tolist()] == e
        assert (src[i, len(e):] == -1).all() and (dets[i, len(e):] == -1).all()
        for j, (v, r) in enumerate(e):
            ox, oy = c['views'][v][1:]
            row = c['dets'][v, r]
            assert dets[i, j].tobytes() == np.array([row[0], row[1], row[2] + F(ox), row[3] + F(oy), row[4] + F(ox), row[5] + F(oy)], dtype=F).tobytes()


def test_hand_cases_cover_the_list():
    assert sorted(R.hand_cases()) == sorted(HAND_ANSWERS)


def test_signed_zero_keeps_its_bits():
    dets, count, _ = R.run(R.hand_cases()['signed_zero'])
    assert np.signbit(dets[0, :4, 1]).tolist() == [True, True, False, True]


def test_translation_is_one_float32_rounding():
    # 0.1 + 3 is not representable: the sum is rounded once, in float32
    c = R.case([[(0, .9, 0.1, 0.2, 10.3, 10.4)]], [(0, 3, 16777217)], 1)
    dets, count, _ = R.run(c)
    assert count.tolist() == [1]
    assert dets[0, 0, 2] == F(F(0.1) + F(3)) and dets[0, 0, 3] == F(F(0.2) + F(16777216.0)) and dets[0, 0, 5] == F(F(10.4) + F(16777216.0))


def test_ios_is_intersection_over_the_smaller_box():
    a, b = np.array([0, 0, 10, 10], dtype=F), np.array([[5, 0, 25, 10], [20, 0, 30, 10], [10, 0, 30, 10]], dtype=F)
    assert R.ios(a, b).tolist() == [0.5, 0.0, 0.0]
    assert R.ios(b[0], a[None]).tolist() == [0.5]


# ---- fairness of the seeded cases ---------------------------------------------------------------------------------------------

def _stats(c, **kw):
    st = []
    R.run(c, stats=st, **kw)
    return st


@pytest.mark.parametrize('seed', R.SEEDS)
def test_modes_differ_on_the_recipe(seed):
    got = tuple(_stats(R.flat_case(seed), metric=m, class_agnostic=a)[0]['selected'] for m, a in R.MODES)
    assert got == R.MODE_COUNTS[seed]
    assert len(set(got)) == 4


@pytest.mark.parametrize('V,K', R.SPREAD)
def test_spread_cases_select_and_suppress(V, K):
    for seed in R.SEEDS:
        c = R.spread_case(seed, V, K)
        assert int(c['count'].sum()) == min(700, V * K) and c['count'].max() <= K
        sel = []
        for m, a in R.MODES:
            st = _stats(c, metric=m, class_agnostic=a)[0]
            assert st['selected'] >= 1 and st['suppressed'] >= 1, (seed, m, a, st)
            sel.append(st['selected'])
        if (V, K) == (41, 100):          # the whole recipe: the four modes give four different selection counts, and the cuts cut
            assert len(set(sel)) == 4, sel
            assert min(sel) > 1 and sel[0] > 40 and sel[2] > 40, sel


@pytest.mark.parametrize('R_,V,K', R.BOUNDARIES)
def test_boundary_cases_admit_exactly_their_rows(R_, V, K):
    c = R.uniform_case(R_, V, K)
    st = _stats(c)[0]
    assert st['admitted'] == R_ == V * K
    assert st['selected'] >= 1 and st['suppressed'] >= 1
    if R_ == R.MAX_ROWS:
        assert st['selected'] > 1024          # the keep_top_k = 1024 cut of this case cuts


def test_boundaries_are_the_kernels_stages():
    from ppyolo_hip import _lib
    assert (R.CHUNK, R.RANK_MAX, R.MAX_ROWS) == (_lib.MERGE_CHUNK, _lib.MERGE_RANK_MAX, _lib.MERGE_MAX_ROWS)
    rows = [b[0] for b in R.BOUNDARIES]
    assert rows == [R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, R.RANK_MAX - 1, R.RANK_MAX, R.RANK_MAX + 1, R.MAX_ROWS]
    assert R.TOO_MANY[0] == R.MAX_ROWS + 1 == R.TOO_MANY[1] * R.TOO_MANY[2]
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ppyolo_hip.h')).read()
    for name, val in (('MAX_ROWS', R.MAX_ROWS), ('RANK_MAX', R.RANK_MAX), ('CHUNK', R.CHUNK), ('MAX_KEEP', _lib.MERGE_MAX_KEEP)):
        assert int(re.search(r'#define PPY_MERGE_%s (\d+)' % name, text).group(1)) == val


def test_interleaved_table_equals_the_images_alone():
    c = R.interleaved_case()
    assert c['views'][:, 0].tolist() == [0, 1] * 5
    dets, count, src = R.run(c)
    for i, seed in enumerate((0, 1)):
        d1, c1, s1 = R.run(R.spread_case(seed, 5, 100))
        assert count[i] == c1[0] >= 1 and dets[i].tobytes() == d1[0].tobytes()
        k = int(c1[0])
        assert (src[i, :k, 0] == 2 * s1[0, :k, 0] + i).all() and (src[i, :k, 1] == s1[0, :k, 1]).all()


def test_batch_case_shape():
    c = R.batch_case()
    st = _stats(c)
    assert [s['admitted'] for s in st] == [0, 0, R.MAX_ROWS]
    assert (c['views'][:, 0] == 0).sum() == 2 and (c['views'][:, 0] == -1).sum() == 3 and (c['views'][:, 0] == 1).sum() == 0
    dets, count, src = R.run(c)
    assert count.tolist() == [0, 0, 1024] and (dets[:2] == -1).all() and (src[:2] == -1).all()


# ---- refusals the host decides ------------------------------------------------------------------------------------------------

def _refusal(V=2, K=4, views=None, n=1, metric=0, thresh=0.5, score_thresh=0.1, keep_top_k=10):
    """The library's own validation.  No workspace is passed, so a call that passes every check ends with PPY_ERR_WORKSPACE (-3):
    nothing here can reach the device, and the device pointers are never read."""
    from ppyolo_hip import _lib
    tab = np.ascontiguousarray(np.zeros((V, 3), dtype=np.int32) if views is None else np.asarray(views, dtype=np.int32))
    reason = ctypes.create_string_buffer(96)
    fake = 1 << 20          # a non-null address
    rc = _lib.lib().ppy_merge_views_f32(fake, fake, V, K, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), fake, n, metric, thresh,
                                        score_thresh, 0, keep_top_k, fake, fake, fake, None, 0, reason, None)
    return rc, reason.value.decode()


@pytest.mark.parametrize('kw,word', [(dict(keep_top_k=0), 'keep_top_k = 0'), (dict(keep_top_k=1025), 'keep_top_k = 1025'),
                                     (dict(K=0), 'K = 0'), (dict(thresh=float('nan')), 'thresh is NaN'),
                                     (dict(score_thresh=float('nan')), 'score_thresh is NaN'), (dict(metric=2), 'metric code 2'),
                                     (dict(V=3, K=2731), '3 views x 2731 rows = 8193 rows'),
                                     (dict(V=8193, K=1), '8193 views x 1 rows = 8193 rows')])
def test_library_refuses_by_name(kw, word):
    import __graft_entry__ as ge
    ge.build()
    rc, reason = _refusal(**kw)
    assert rc == -2 and word in reason, (rc, reason)


def test_library_counts_rows_per_image_not_per_call():
    import __graft_entry__ as ge
    ge.build()
    # 8193 views of K = 1 in all, but image 1 has one of them and 100 are padding: image 0 stays inside the limit
    views = np.zeros((8193, 3), dtype=np.int32)
    views[5, 0] = 1
    views[100:200, 0] = -1
    assert _refusal(V=8193, K=1, views=views, n=2) == (-3, '')          # every limit passed: only the workspace is missing
    views[5, 0] = 2                                      # image 2 of n = 2
    assert _refusal(V=8193, K=1, views=views, n=2)[0] == -1
    assert _lib_bytes(1, 41, 100) == 32 * 4100 and _lib_bytes(2, 8193, 1) == 2 * 32 * 8192 and _lib_bytes(0, 1, 1) == 0


def _lib_bytes(n, V, K):
    from ppyolo_hip import _lib
    return _lib.lib().ppy_merge_views_workspace_bytes(n, V, K)


def test_wrapper_and_detector_refuse_by_name():
    from ppyolo_hip import ops, tiles
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError, match="unknown metric 'giou'"):
        ops.merge_views(None, None, None, None, 1, 'giou', 0.5, 0.1, False, 10, None, None, None)
    with pytest.raises(PPYoloHipError, match='does not fit int32'):
        ops.merge_views_table([(0, 1 << 31, 0)])
    assert ops.merge_views_table([(0, 1, 2), (-1, 3, 4)]).tolist() == [[0, 1, 2], [-1, 3, 4]]

    class Cfg(object):
        nms_cfg = dict(post_threshold=0.01, keep_top_k=100)
    for kw, word in [(dict(metric='giou'), 'unknown metric'), (dict(thresh=float('nan')), 'thresh is NaN'),
                     (dict(score_thresh=float('nan')), 'score_thresh is NaN'), (dict(keep_top_k=0), 'keep_top_k = 0'),
                     (dict(keep_top_k=1025), 'keep_top_k = 1025'), (dict(overlap=1.0), 'overlap'), (dict(tile=0), 'tile'),
                     (dict(batch=0), 'batch')]:
        with pytest.raises(PPYoloHipError, match=word):
            tiles.TiledDetector(None, Cfg(), 64, **kw)
