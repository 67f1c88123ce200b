"""The numpy restatement of the weighted boxes fusion (tests/fuse_views_ref.py) on answers worked out by hand, with the
arithmetic written here; what the seeded cases of tests/test_gpu_fuse_views.py exercise; plan_tta_views; and every refusal the
host decides (the library's validation runs before anything touches the device)."""
import ctypes

import numpy as np
import pytest

import fuse_views_ref as R

F = np.float32


def one(name, **kw):
    """A hand case -> (its clusters of image 0 as (class, conf, box, (view, row), members), stats)."""
    c = R.hand_cases()[name]
    p = dict(c['kw'])
    p.pop('keep_top_k')
    p.update(kw)
    st = {}
    return c, R.fuse_image(c['dets'], c['count'], c['views'], c['weight'], 0, stats=st, **p), st


def wmean(pairs):
    """[(s, coordinate)] -> X / S in float32, products rounded, then the running sum: the contract's arithmetic."""
    S, X = F(pairs[0][0]), F(F(pairs[0][0]) * F(pairs[0][1]))
    for s, b in pairs[1:]:
        S = F(S + F(s))
        X = F(X + F(F(s) * F(b)))
    return F(X / S), S


def test_two_equal_boxes_from_two_views():
    _, cl, st = one('equal_boxes')
    assert len(cl) == 1 and st == dict(admitted=2, clusters=1, max_members=2, singletons=0, classes=1)
    cls, conf, box, first, members = cl[0]
    # S = .8 + .6; every coordinate (.8 b + .6 b) / 1.4 = b up to float32 rounding; T = 2 = wsum: conf = ((S / 2) * 2) / 2 = .7
    S = F(F(.8) + F(.6))
    assert (cls, first, members) == (1, (0, 0), 2)
    assert conf == F(F(F(S / F(2)) * F(2)) / F(2)) and abs(float(conf) - 0.7) < 1e-6
    assert box.tolist() == [wmean([(.8, b), (.6, b)])[0] for b in (10, 10, 50, 50)]
    assert np.allclose(box, [10, 10, 50, 50], rtol=0, atol=1e-5)


def test_singleton_among_two_views():
    c, cl, st = one('singleton_of_two_views')
    cls, conf, box, first, members = cl[0]
    # q = .8 / 1, m = min(1, 2) = 1, conf = (.8 * 1) / 2
    assert members == 1 and conf == F(F(.8) / F(2)) and box.tobytes() == c['dets'][0, 0, 2:6].tobytes()
    assert st['singletons'] == 1


def test_weighted_mean_of_two_boxes():
    _, cl, _ = one('weighted_mean')
    # IoU = 8 * 10 / (100 + 100 - 80) = 2 / 3 > .55.  x0 = (.9 * 0 + .3 * 2) / 1.2 = .5, x1 = (9 + 3.6) / 1.2 = 10.5
    assert len(cl) == 1 and cl[0][4] == 2
    assert cl[0][2].tolist() == [wmean([(.9, a), (.3, b)])[0] for a, b in ((0, 2), (0, 0), (10, 12), (10, 10))]
    assert np.allclose(cl[0][2], [0.5, 0, 10.5, 10], rtol=0, atol=1e-6)
    assert abs(float(cl[0][1]) - 0.6) < 1e-6          # ((1.2 / 2) * 2) / 2


def test_a_row_is_matched_against_the_fused_box_not_the_members():
    """thresh .4.  A = (0, 0, 10, 16) and B = (0, 0, 16, 10), both .8: IoU = 100 / (160 + 160 - 100) = .4545, one cluster, fused
    (0, 0, 13, 13).  C = (3, 3, 13, 13) at .5: with the fused box 100 / 169 = .592; with A 7 * 10 / (100 + 160 - 70) = .368, with B
    the same: C joins because of the fused box alone.  The three fuse to x0 = y0 = 1.5 / 2.1 = .714, x1 = y1 = 27.3 / 2.1 = 13.
    D = (0, 6, 10, 16) at .4: with A 100 / 160 = .625, but with the fused box 9.286 * 7 / (100 + 150.94 - 65) = .3497: D opens a
    cluster of its own."""
    A, B, C, D = (F([0, 0, 10, 16]), F([0, 0, 16, 10]), F([3, 3, 13, 13]), F([0, 6, 10, 16]))
    thr = F(0.4)
    assert R.iou(B, A) > thr
    AB = F([0, 0, 13, 13])
    assert R.iou(C, AB) > thr and not R.iou(C, A) > thr and not R.iou(C, B) > thr
    assert abs(float(R.iou(C, AB)) - 100 / 169) < 1e-6 and abs(float(R.iou(C, A)) - 70 / 190) < 1e-6
    _, cl, st = one('fused_not_members')
    assert [(t[3], t[4]) for t in cl] == [((0, 0), 3), ((1, 1), 1)] and st['max_members'] == 3 and st['singletons'] == 1
    ABC = cl[0][2]
    assert np.allclose(ABC, [1.5 / 2.1, 1.5 / 2.1, 13, 13], rtol=0, atol=1e-5)
    assert R.iou(D, A) > thr and not R.iou(D, ABC) > thr and abs(float(R.iou(D, ABC)) - 0.3497) < 1e-3
    assert cl[1][2].tobytes() == D.tobytes()
    # had D been matched against the members, the cluster would hold all four rows
    _, cl2, _ = one('fused_not_members', thresh=0.3)
    assert [t[4] for t in cl2] == [4]


def test_an_iou_equal_to_thresh_does_not_join():
    # (0, 0, 3, 1) and (1, 0, 4, 1): 2 / (3 + 3 - 2) = .5 exactly
    assert R.iou(F([1, 0, 4, 1]), F([0, 0, 3, 1])) == F(0.5)
    _, cl, _ = one('iou_equal_to_thresh')
    assert [t[4] for t in cl] == [1, 1]
    _, cl, _ = one('iou_equal_to_thresh', thresh=float(np.nextafter(F(0.5), F(0))))
    assert [t[4] for t in cl] == [2]


def test_a_tie_goes_to_the_earlier_cluster():
    # (0, 0, 10, 10) and (4, 0, 14, 10): 60 / 140 < .55, two clusters; (2, 0, 12, 10) meets both at 80 / 120
    a, b, r = F([0, 0, 10, 10]), F([4, 0, 14, 10]), F([2, 0, 12, 10])
    assert R.iou(r, a) == R.iou(r, b) > F(0.55) and not R.iou(b, a) > F(0.55)
    _, cl, _ = one('tie_goes_to_the_earlier')
    assert [(t[3], t[4]) for t in cl] == [((0, 0), 2), ((0, 1), 1)]


def test_three_rows_of_one_view_members_above_wsum():
    _, cl, _ = one('one_view_three_rows')
    # T = 3 > wsum = 1: m = 1, conf = ((S / 3) * 1) / 1: the mean of the scores
    S = F(F(F(.9) + F(.6)) + F(.3))
    assert len(cl) == 1 and cl[0][4] == 3 and cl[0][1] == F(F(F(S / F(3)) * F(1)) / F(1)) and abs(float(cl[0][1]) - 0.6) < 1e-6


def test_the_same_box_in_two_classes():
    _, cl, st = one('two_classes')
    assert [(t[0], t[4]) for t in cl] == [(1, 1), (2, 1)] and st['classes'] == 2
    assert cl[0][2].tolist() == cl[1][2].tolist() == [13, 14, 53, 54]          # the view's origin (3, 4) added


def test_a_view_weight_of_two():
    _, cl, _ = one('view_weight_two')
    # s = .4 * 2 = .8 and .6 * 1: the weighted view's row comes first.  x0 = (.6 * 2) / 1.4; wsum = 3: conf = ((1.4 / 2) * 2) / 3
    s0, s1 = F(F(.4) * F(2)), F(F(.6) * F(1))
    S = F(s0 + s1)
    assert cl[0][3] == (0, 0) and cl[0][4] == 2
    assert cl[0][2][0] == F(F(F(s0 * F(0)) + F(s1 * F(2))) / S) and abs(float(cl[0][2][0]) - 1.2 / 1.4) < 1e-6
    assert cl[0][1] == F(F(F(S / F(2)) * F(2)) / F(3)) and abs(float(cl[0][1]) - 1.4 / 3) < 1e-6


def test_mirror_then_origin():
    assert R.transform(F([0, .9, 10, 5, 30, 20]), (0, 0, 0, 100)).tolist() == [70, 5, 90, 20]
    _, cl, _ = one('mirror')
    assert cl[0][2].tolist() == [77, 14, 97, 29]          # (70, 5, 90, 20) + (7, 9)
    _, cl, _ = one('mirror_joins')
    assert [t[4] for t in cl] == [2] and np.allclose(cl[0][2], [70, 5, 90, 20], rtol=0, atol=1e-4)


def test_every_inadmissible_row_kind_is_rejected():
    c, cl, st = one('left_out')
    assert st['admitted'] == 5 and sorted(t[3] for t in cl) == [(0, 0), (2, 1), (3, 2), (4, 1), (4, 2)]
    _, cl, st = one('score_thresh')
    assert [t[3] for t in cl] == [(0, 0), (0, 2)]          # .29 is out, .3 is in
    _, cl, st = one('padding_view')
    assert st['admitted'] == 2 and cl[0][3] == (2, 0) and cl[0][1] == F(F(F(F(F(.6) + F(.5)) / F(2)) * F(2)) / F(2))


def test_output_order_on_equal_conf_and_the_cut():
    _, cl, _ = one('order_on_equal_conf')
    # the class-0 pair: ((.5 / 2) * 2) / 2 = .25 = every singleton's .5 / 2: class ascending, then creation order
    assert [(t[0], float(t[1]), t[3]) for t in cl] == [(0, .25, (0, 3)), (1, .25, (0, 1)), (1, .25, (0, 2)), (2, .25, (0, 0))]
    c = R.hand_cases()['cut']
    dets, count, src, members = R.run(c)
    assert count.tolist() == [3] and src[0].tolist() == [[1, 1], [1, 0], [0, 2]] and members[0].tolist() == [1, 1, 1]
    full = R.run(c, keep_top_k=8)
    assert full[1].tolist() == [5] and full[0][0, :3].tobytes() == dets[0].tobytes() and (full[0][0, 5:] == -1).all()
    assert (full[2][0, 5:] == -1).all() and (full[3][0, 5:] == -1).all()


def test_an_image_without_a_view_and_empty_inputs():
    c = R.hand_cases()['image_without_view']
    dets, count, src, members = R.run(c)
    assert count.tolist() == [1, 0, 1] and members[:, 0].tolist() == [2, -1, 1] and src[2, 0].tolist() == [0, 0]
    assert R.run(R.hand_cases()['no_rows'])[1].tolist() == [0]
    assert R.run(R.hand_cases()['one_row'])[3][0, :2].tolist() == [1, -1]


def test_running_sums_stay_float32():
    """A float64 anywhere in S or X would round differently on this input: 0.1 + 0.2 + 0.3 in float32 steps."""
    c = R.case([[(0, .1, 0, 0, 10, 10), (0, .2, 0, 0, 10, 10), (0, .3, 0, 0, 10, 10)]], [(0, 0, 0, 0)], 1)
    cl = R.fuse_image(c['dets'], c['count'], c['views'], c['weight'], 0)
    S = F(F(F(.3) + F(.2)) + F(.1))
    assert cl[0][1].dtype == F and cl[0][2].dtype == F and cl[0][1] == F(F(F(S / F(3)) * F(1)) / F(1))


# ---- what the seeded cases exercise -----------------------------------------------------------------------------------------------

def mixed(st):
    return st['max_members'] >= 2 and st['singletons'] >= 1


@pytest.mark.parametrize('V', R.SPREAD_V)
def test_spread_cases_join_and_leave_singletons(V):
    c = R.spread_case(V % 4, V)
    st = []
    R.run(c, stats=st)
    assert mixed(st[0]) and (c['views'][:, 3] > 0).sum() == V // 2
    # the mirrors change where the rows are stored, not where they land
    plain = R.spread_case(V % 4, V, mirror=False)
    a, b = R.run(c), R.run(plain)
    assert a[1].tolist() == b[1].tolist() and a[3].tobytes() == b[3].tobytes() and np.allclose(a[0], b[0], rtol=0, atol=2e-3)


@pytest.mark.parametrize('rows,V,K', R.BOUNDARIES[:-1])
def test_boundary_cases_admit_exactly_their_rows(rows, V, K):
    st = []
    R.run(R.uniform_case(rows, V, K), stats=st)
    assert st[0]['admitted'] == rows == V * K and mixed(st[0])


def test_the_large_cases():
    st = []
    R.run(R.uniform_case(*R.BOUNDARIES[-1]), stats=st)
    assert st[0]['admitted'] == R.MAX_ROWS and st[0]['clusters'] > 1024 and mixed(st[0])
    st = []
    R.run(R.one_class_case(), stats=st)
    assert st[0]['admitted'] == 2048 and st[0]['classes'] == 1 and mixed(st[0])
    st = []
    R.run(R.many_classes_case(), stats=st)
    assert st[0]['classes'] == 80 and mixed(st[0])
    for V, K in R.MANY_VIEWS:
        c = R.many_views_case(V, K)
        st = []
        R.run(c, stats=st)
        assert mixed(st[0]) and (c['views'][:, 0] == -1).sum() == V // 4
    st = []
    R.run(R.poisoned_case(), stats=st)
    assert mixed(st[0]) and mixed(st[1])


# ---- the view plan ----------------------------------------------------------------------------------------------------------------

def test_plan_tta_views():
    from ppyolo_hip.tta import plan_tta_views
    sizes = [(480, 640), (427, 500), (100, 50)]
    plan = plan_tta_views(sizes, (512, 608), True, 8)
    one_scale = [(0, 0, 640), (0, 1, 640), (1, 0, 500), (1, 1, 500), (2, 0, 50), (2, 1, 50), (-1, 0, 0), (-1, 0, 0)]
    assert plan == [(i, si, f, w if f else 0) for si in (0, 1) for i, f, w in one_scale]
    assert [r for r in plan if r[0] >= 0] == R.tta_views(sizes, (512, 608), True)
    assert plan_tta_views(sizes, (64,), False, 2) == [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (-1, 0, 0, 0)]
    assert len(plan_tta_views([(480, 640)] * 8, (512, 608, 704), True, 8)) == 48          # six chunks, none padded
    assert plan_tta_views(sizes[:1], (64,), False, 1) == [(0, 0, 0, 0)]


# ---- refusals the host decides ----------------------------------------------------------------------------------------------------

def _refusal(V=2, K=4, views=None, weight=None, n=1, thresh=0.5, score_thresh=0.1, keep_top_k=10):
    """The library's own validation.  No workspace is passed, so a call that passes every check ends with PPY_ERR_WORKSPACE (-3):
    nothing here can reach the device, and the device pointers are never read."""
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    tab = np.ascontiguousarray(np.zeros((V, 4), dtype=np.int32) if views is None else np.asarray(views, dtype=np.int32))
    w = np.ascontiguousarray(np.ones((V,), dtype=np.float32) if weight is None else np.asarray(weight, dtype=np.float32))
    reason = ctypes.create_string_buffer(96)
    fake = 1 << 20          # a non-null address
    rc = _lib.lib().ppy_fuse_views_f32(fake, fake, V, K, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), fake,
                                       w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), fake, n, thresh, score_thresh, keep_top_k,
                                       fake, fake, fake, fake, None, 0, reason, None)
    return rc, reason.value.decode()


@pytest.mark.parametrize('kw,word', [(dict(keep_top_k=0), 'keep_top_k = 0'), (dict(keep_top_k=1025), 'keep_top_k = 1025'),
                                     (dict(K=0), 'K = 0'), (dict(thresh=float('nan')), 'thresh is NaN'),
                                     (dict(score_thresh=float('nan')), 'score_thresh is NaN'),
                                     (dict(V=3, K=2731), '3 views x 2731 rows = 8193 rows'),
                                     (dict(V=8193, K=1), '8193 views x 1 rows = 8193 rows'),
                                     (dict(weight=[1, float('nan')]), 'view 1: weight nan'), (dict(weight=[0, 1]), 'view 0: weight 0'),
                                     (dict(weight=[1, float('inf')]), 'view 1: weight inf'), (dict(weight=[1, -2]), 'view 1: weight -2'),
                                     (dict(views=[(0, 0, 0, 0), (0, 0, 0, -3)]), 'view 1: mirror_w = -3')])
def test_library_refuses_by_name(kw, word):
    rc, reason = _refusal(**kw)
    assert rc == -2 and word in reason, (rc, reason)


def test_library_ignores_padding_views_and_counts_rows_per_image():
    views = np.zeros((8193, 4), dtype=np.int32)
    views[5, 0] = 1
    views[100:200] = (-1, 0, 0, -9)                      # a padding view's mirror width and weight are never looked at
    weight = np.ones((8193,), dtype=np.float32)
    weight[100:200] = np.nan
    assert _refusal(V=8193, K=1, views=views, weight=weight, n=2) == (-3, '')      # every limit passed: only the workspace is missing
    views[5, 0] = 2                                      # image 2 of n = 2
    assert _refusal(V=8193, K=1, views=views, weight=weight, n=2)[0] == -1
    from ppyolo_hip import _lib
    b = _lib.lib().ppy_fuse_views_workspace_bytes
    assert b(1, 41, 100) == 64 * 4100 and b(2, 8193, 1) == 2 * 64 * 8192 and b(0, 1, 1) == 0


def test_wrapper_and_detector_refuse_by_name():
    from ppyolo_hip import ops, tta
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError, match='does not fit int32'):
        ops.fuse_views_table([(0, 1 << 31, 0, 0)])
    assert ops.fuse_views_table([(0, 1, 2, 0), (-1, 3, 4, 5)]).tolist() == [[0, 1, 2, 0], [-1, 3, 4, 5]]

    class Cfg(object):
        nms_cfg = dict(post_threshold=0.01, keep_top_k=100)
        head = dict(downsample=[32, 16])
    for kw, word in [(dict(scales=()), 'at least one network input side'), (dict(scales=(64, 100)), 'scale 100'),
                     (dict(scales=(0,)), 'scale 0'), (dict(scales=5), 'expected a sequence'),
                     (dict(thresh=float('nan')), 'thresh is NaN'), (dict(score_thresh=float('nan')), 'score_thresh is NaN'),
                     (dict(keep_top_k=0), 'keep_top_k = 0'), (dict(keep_top_k=1025), 'keep_top_k = 1025'), (dict(batch=0), 'batch'),
                     (dict(weights=[[1, 1]]), r'expected 2 rows \(one per scale\) of 2 values'),
                     (dict(weights=[1, [1, 2, 3]]), 'expected 2 rows'), (dict(hflip=False, weights=[[1, 1], [1, 1]]), 'of 1 values'),
                     (dict(weights=[1, 0]), 'finite and positive'), (dict(weights=[[1, float('nan')], 1]), 'finite and positive'),
                     (dict(weights=[[1, float('inf')], 1]), 'finite and positive')]:
        args = dict(scales=(64, 96))
        args.update(kw)
        with pytest.raises(PPYoloHipError, match=word):
            tta.TtaDetector(None, Cfg(), **args)
    with pytest.raises(PPYoloHipError, match='empty batch'):
        tta.plan_tta_views([], (64,))
    with pytest.raises(PPYoloHipError, match='batch'):
        tta.plan_tta_views([(4, 4)], (64,), True, 0)
