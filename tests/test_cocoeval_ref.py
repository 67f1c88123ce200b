"""The float64 COCOeval restatement (tests/cocoeval_ref.py) on answers derived by hand -- it is the oracle of the device
evaluator, and pycocotools is not installed here to pin it.  CASES are shared with tests/test_gpu_cocoeval.py, which runs
each one through the device."""
import numpy as np
import pytest

import cocoeval_ref as R

EPS = np.spacing(1)
LONE_TP = 1.0 / (1.0 + EPS)         # 0.9999999999999998


def _gt(boxes, images=(1,), cats=(1,), areas=None, crowd=None, ids=None, img=None, cat=None):
    anns = []
    for j, b in enumerate(boxes):
        anns.append({'id': ids[j] if ids else j + 1, 'image_id': img[j] if img else images[0],
                     'category_id': cat[j] if cat else cats[0], 'bbox': list(b),
                     'area': areas[j] if areas else b[2] * b[3], 'iscrowd': crowd[j] if crowd else 0})
    return {'images': [{'id': i} for i in images], 'categories': [{'id': c} for c in cats], 'annotations': anns}


def _dt(img, cat, box, score):
    return {'image_id': img, 'category_id': cat, 'bbox': list(box), 'score': score}


def case_perfect():
    g = _gt([[0, 0, 50, 50], [10, 10, 200, 100]], images=(1, 2), img=[1, 2])
    return g, [_dt(1, 1, [0, 0, 50, 50], .9), _dt(2, 1, [10, 10, 200, 100], .8)]


def case_lone_tp():
    return _gt([[0, 0, 50, 50]]), [_dt(1, 1, [0, 0, 50, 50], .9)]


def case_fp_above_tp():
    return _gt([[0, 0, 50, 50]]), [_dt(1, 1, [500, 500, 20, 20], .9), _dt(1, 1, [0, 0, 50, 50], .8)]


def case_iou_half():
    return _gt([[0, 0, 10, 10]]), [_dt(1, 1, [0, 0, 10, 20], .7)]


def case_equal_iou_later_gt():
    # two GTs with the same box; the later one (annotation id 0) is taken, and a match to id 0 reads as unmatched
    return _gt([[0, 0, 40, 40], [0, 0, 40, 40]], ids=[7, 0]), [_dt(1, 1, [0, 0, 40, 40], .9)]


def case_crowd():
    g = _gt([[0, 0, 100, 100], [300, 300, 40, 40]], crowd=[1, 0])
    d = [_dt(1, 1, [10, 10, 20, 20], .95), _dt(1, 1, [50, 50, 30, 30], .9), _dt(1, 1, [0, 0, 100, 100], .85),
         _dt(1, 1, [300, 300, 40, 40], .5)]
    return g, d


def case_area_1024():
    return _gt([[0, 0, 32, 32]], areas=[1024]), [_dt(1, 1, [0, 0, 32, 32], .9)]


def case_truncation():
    # image 1: one GT, 150 detections, the TP ranked 120th; image 2: the TP ranked 5th; image 3: the TP ranked 0th
    g = _gt([[0, 0, 60, 60]] * 3, images=(1, 2, 3), img=[1, 2, 3])
    d = []
    for j in range(150):
        d.append(_dt(1, 1, [0, 0, 60, 60] if j == 120 else [1000 + j, 0, 10, 10], 1.0 - j / 1000))
    for j in range(8):
        d.append(_dt(2, 1, [0, 0, 60, 60] if j == 5 else [0, 1000 + j, 10, 10], 0.9 - j / 100))
    d.append(_dt(3, 1, [0, 0, 60, 60], 0.3))
    return g, d


def case_tie_across_images():
    # images listed out of order; equal scores: image 1's FP comes before image 2's TP
    g = _gt([[0, 0, 50, 50], [0, 0, 50, 50]], images=(2, 1), img=[1, 2])
    return g, [_dt(2, 1, [0, 0, 50, 50], .5), _dt(1, 1, [400, 400, 50, 50], .5)]


def case_category_without_gt():
    g = _gt([[0, 0, 50, 50]], cats=(1, 2))
    return g, [_dt(1, 1, [0, 0, 50, 50], .9), _dt(1, 2, [0, 0, 50, 50], .8), _dt(1, 3, [0, 0, 50, 50], .8)]


def case_image_without_gt():
    g = _gt([[0, 0, 50, 50]], images=(1, 2))
    return g, [_dt(1, 1, [0, 0, 50, 50], .5), _dt(2, 1, [0, 0, 50, 50], .9)]


CASES = {f.__name__[5:]: f for f in [case_perfect, case_lone_tp, case_fp_above_tp, case_iou_half, case_equal_iou_later_gt,
                                     case_crowd, case_area_1024, case_truncation, case_tie_across_images,
                                     case_category_without_gt, case_image_without_gt]}


def run(name):
    g, d = CASES[name]()
    p, r, s = R.evaluate(g, d)
    return p, r, s, R.summarize(p, r)


def test_params_are_pycocotools_defaults():
    assert np.array_equal(R.IOU_THRS, np.linspace(.5, .95, 10)) and np.array_equal(R.REC_THRS, np.linspace(0, 1, 101))
    assert R.MAX_DETS == [1, 10, 100] and R.AREA_RNG == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_perfect_detections():
    p, r, s, st = run('perfect')
    assert st[0] == 1.0 and st[1] == 1.0 and st[8] == 1.0          # two TPs: p_2 = 2 / (2 + eps) rounds to exactly 1
    assert np.all(p[:, :, 0, 0, 2] == 1.0) and np.all(r[:, 0, 0, 2] == 1.0)


def test_lone_tp_is_one_over_one_plus_eps():
    p, r, s, st = run('lone_tp')
    assert LONE_TP == 0.9999999999999998
    assert np.all(p[:, :, 0, 0, :] == LONE_TP) and st[0] == LONE_TP and st[8] == 1.0
    assert np.all(s[:, :, 0, 0, :] == .9)


def test_fp_above_tp_gives_half():
    p, r, s, st = run('fp_above_tp')
    assert np.all(p[:, :, 0, 0, 1:] == 0.5) and st[0] == 0.5
    assert np.all(p[:, :, 0, 0, 0] == 0.0) and np.all(r[:, 0, 0, 0] == 0.0)        # maxDets 1 keeps the FP only
    assert np.all(s[:, 0, 0, 0, 2] == .9) and np.all(s[:, 1:, 0, 0, 2] == .8)


def test_iou_of_exactly_half_matches_at_050():
    assert R.bb_iou([0, 0, 10, 20], [0, 0, 10, 10], 0) == 0.5
    p, r, s, st = run('iou_half')
    assert np.all(p[0, :, 0, 0, 2] == LONE_TP) and np.all(p[1:, :, 0, 0, 2] == 0.0)
    assert r[0, 0, 0, 2] == 1.0 and np.all(r[1:, 0, 0, 2] == 0.0)


def test_equal_iou_takes_the_later_gt():
    g, d = CASES['equal_iou_later_gt']()
    gts = [dict(a, ignore=0) for a in g['annotations']]
    e = R.evaluate_img(gts, R.load_res(g, d), R.AREA_RNG[0], 100)
    assert np.all(e['dtMatches'] == 0)                  # matched to the later GT, whose id is 0: pycocotools' "no match"
    p, r, s, st = run('equal_iou_later_gt')
    assert np.all(p[:, :, 0, 0, 2] == 0.0) and np.all(r[:, 0, 0, 2] == 0.0)


def test_crowd_absorbs_detections():
    p, r, s, st = run('crowd')
    # three detections inside the crowd region are ignored (neither TP nor FP); the lone TP ranks last
    assert np.all(p[:, :, 0, 0, 2] == LONE_TP) and np.all(r[:, 0, 0, 2] == 1.0)
    assert np.all(s[:, 1:, 0, 0, 2] == .5) and np.all(s[:, 0, 0, 0, 2] == .95)


def test_area_1024_is_small_and_medium():
    p, r, s, st = run('area_1024')
    assert np.all(p[:, :, 0, 1, 2] == LONE_TP) and np.all(p[:, :, 0, 2, 2] == LONE_TP) and np.all(p[:, :, 0, 3, :] == -1)
    assert st[3] == LONE_TP and st[4] == LONE_TP and st[5] == -1


def test_max_dets_truncate_per_pair():
    p, r, s, st = run('truncation')
    assert np.all(r[:, 0, 0, 0] == 1 / 3)               # maxDets 1: image 3's TP only
    assert np.all(r[:, 0, 0, 1] == 2 / 3)               # maxDets 10: images 2 and 3
    assert np.all(r[:, 0, 0, 2] == 2 / 3)               # maxDets 100: image 1's TP (rank 120) is cut


def test_score_ties_break_by_image_id():
    p, r, s, st = run('tie_across_images')
    # image 1's FP first, then image 2's TP: precision 0.5 up to recall 0.5 (npig 2), 0 beyond
    assert np.all(p[:, :51, 0, 0, 2] == 0.5) and np.all(p[:, 51:, 0, 0, 2] == 0.0)


def test_category_without_gt_is_minus_one_and_excluded():
    p, r, s, st = run('category_without_gt')
    assert p.shape[2] == 2 and np.all(p[:, :, 1] == -1) and np.all(r[:, 1] == -1) and np.all(s[:, :, 1] == -1)
    assert st[0] == LONE_TP and st[8] == 1.0


def test_image_without_gt_contributes_fps():
    p, r, s, st = run('image_without_gt')
    assert np.all(p[:, :, 0, 0, 2] == 0.5) and np.all(r[:, 0, 0, 2] == 1.0)


def test_result_on_unknown_image_and_nan_are_rejected():
    g, d = CASES['lone_tp']()
    with pytest.raises(ValueError):
        R.evaluate(g, d + [_dt(99, 1, [0, 0, 1, 1], .5)])
    with pytest.raises(ValueError):
        R.evaluate(g, [_dt(1, 1, [0, 0, float('nan'), 1], .5)])


def test_summary_lines_format():
    p, r, s, st = run('perfect')
    lines = []
    R.summarize(p, r, lines)
    assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000'
    assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000'
    assert lines[3] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000'
