"""multiclass_nms without a GPU: the float32 numpy restatement (tests/multiclass_nms_ref.py, the oracle of the GPU tests)
against hand-derived answers, and the head's nms_cfg handling."""
import numpy as np
import pytest

import multiclass_nms_ref as R

F = np.float32


def run(boxes, scores, **kw):
    cfg = dict(score_threshold=0.0, nms_top_k=1024, keep_top_k=1024, nms_threshold=0.5, normalized=True)
    cfg.update(kw)
    return R.multiclass_nms(np.asarray(boxes, dtype=F), np.asarray(scores, dtype=F), **cfg)


def kept_boxes(boxes, scores, **kw):
    C = np.asarray(scores).shape[1]
    return sorted(int(k) // C for k in run(boxes, scores, **kw)[1])


def test_exact_threshold():
    boxes = [[0, 0, 2, 2], [0, 0, 2, 1]]
    scores = [[0.9], [0.8]]
    assert R.iou(F(boxes[0]), F(boxes[1]), True) == F(0.5)
    assert R.iou(F(boxes[0]), F(boxes[1]), False) == F(6) / F(9)
    assert kept_boxes(boxes, scores, nms_threshold=0.5) == [0, 1]            # iou <= threshold keeps
    assert kept_boxes(boxes, scores, nms_threshold=0.49) == [0]
    assert kept_boxes(boxes, scores, nms_threshold=0.5, normalized=False) == [0]
    # the threshold is rounded to float32 before the compare: 0.5 + 1e-9 is 0.5 there, 0.5 - 1e-9 is 0.5 too
    assert kept_boxes(boxes, scores, nms_threshold=0.5 - 1e-9) == [0, 1]
    # float32(6/9) = 0.6666667 > 2/3 as a double: kept only because the threshold is rounded to the same float32
    assert kept_boxes(boxes, scores, nms_threshold=2.0 / 3.0, normalized=False) == [0, 1]


@pytest.mark.parametrize('normalized', [True, False])
def test_chain_keeps_the_even_indices(normalized):
    boxes, scores = R.chain(200)
    near = R.iou(boxes[0], boxes[1], normalized)
    far = R.iou(boxes[0], boxes[2], normalized)
    assert abs(float(near) - (0.538 if normalized else 0.571)) < 1e-3
    assert abs(float(far) - (0.25 if normalized else 0.294)) < 1e-3
    # a suppressed box must not suppress: 1 is dropped by 0, so 2 stays, ...
    assert kept_boxes(boxes, scores, nms_threshold=0.45, normalized=normalized) == list(range(0, 200, 2))


def test_chain_truncated_at_nms_top_k():
    boxes, scores = R.chain(1500)
    assert kept_boxes(boxes, scores, nms_threshold=0.45, nms_top_k=1024) == list(range(0, 1024, 2))


def test_nan_iou_suppresses():
    z = [[1, 1, 1, 1], [1, 1, 1, 1]]
    sc = [[0.9], [0.8]]
    assert np.isnan(R.iou(F(z[0]), F(z[1]), True))                            # 0 / 0
    assert kept_boxes(z, sc, normalized=True) == [0]
    assert R.iou(F(z[0]), F(z[1]), False) == F(1)
    assert kept_boxes(z, sc, normalized=False) == [0]
    inv = [[5, 5, 3, 3], [5, 5, 3, 3]]
    assert R.iou(F(inv[0]), F(inv[1]), True) == F(0)                          # disjoint by the first test
    assert kept_boxes(inv, sc, normalized=True) == [0, 1]
    assert kept_boxes(inv, sc, normalized=False) == [0, 1]


def test_ties():
    # inside a class: equal scores go by box index, so box 0 is scanned first and suppresses box 1 (not the reverse)
    boxes = [[0, 0, 10, 10], [0, 0, 10, 9], [50, 50, 60, 60]]
    dets, keep = run(boxes, [[0.5], [0.5], [0.5]], nms_threshold=0.5)
    assert list(keep) == [0, 2]
    # across classes at the keep_top_k cut: equal scores go to the lower class
    far = [[0, 0, 10, 10], [100, 100, 110, 110]]
    sc = [[0.5, 0.5, 0.5], [0.7, 0.0, 0.5]]
    dets, keep = run(far, sc, keep_top_k=3)
    # selections: class 0: (1, .7) (0, .5); class 1: (0, .5); class 2: (0, .5) (1, .5) -> .7, then the first two .5
    assert [(int(d[0]), int(k) // 3) for d, k in zip(dets, keep)] == [(0, 1), (0, 0), (1, 0)]
    assert list(dets[:, 1]) == [F(0.7), F(0.5), F(0.5)]
    # rows come out class ascending, score descending, box ascending -- and carry the original score and box
    dets, keep = run(far, sc, keep_top_k=10)
    assert [(int(d[0]), int(k) // 3) for d, k in zip(dets, keep)] == [(0, 1), (0, 0), (1, 0), (2, 0), (2, 1)]
    assert np.array_equal(dets[0, 2:], F(far[1]))


def test_background_label_and_strict_threshold():
    far = [[0, 0, 10, 10], [100, 100, 110, 110]]
    sc = [[0.9, 0.8], [0.7, 0.25]]
    dets, keep = run(far, sc, background_label=0)
    assert [int(d[0]) for d in dets] == [1, 1]
    dets, keep = run(far, sc, background_label=-1, score_threshold=0.25)      # strict: 0.25 itself does not pass
    assert sorted(int(k) for k in keep) == [0, 1, 2]
    dets, keep = run(far, sc, score_threshold=0.95)
    assert dets.shape == (0, 6) and keep.shape == (0,)
    d, cnt, k = R.padded([(dets, keep)], 4)
    assert cnt[0] == 0 and (d == -1).all() and (k == -1).all()


def test_clustered_recipe_exercises_every_stage():
    """The GPU comparison's input (test 4) truncates every class at nms_top_k, suppresses and cuts at keep_top_k."""
    for seed in (0, 1, 2):
        st = {}
        boxes, scores = R.clustered(seed)
        dets, keep = R.multiclass_nms(boxes, scores, stats=st, **R.CLUSTERED_CFG)
        assert st['truncated'] == 5 and 244 <= st['suppressed'] <= 252 and 68 <= st['selected'] <= 76, st
        assert dets.shape[0] == 40 and (scores == F(0.25)).mean() > 0.15


def _head(nms_cfg):
    from config import PPYOLO_r18vd_Config, select_head
    cfg = PPYOLO_r18vd_Config()
    return select_head(cfg.head_type)(yolo_loss=None, nms_cfg=nms_cfg, **cfg.head)


class _Out(object):
    H = W = 2


def test_head_builds_the_decode_dictionary():
    from config import PPYOLO_r18vd_Config, multiclass_nms_defaults
    hd = _head(multiclass_nms_defaults())
    outs = [_Out() for _ in hd.anchor_masks]
    d = hd.decode_params(outs)
    assert d['nms_type'] == 'multiclass_nms'
    assert d['nms'] == dict(score_threshold=0.01, nms_top_k=1000, keep_top_k=100, nms_threshold=0.45, normalized=False,
                            background_label=-1, nms_eta=1.0)
    # the default configuration is untouched: matrix_nms, the keys the oracle's matrix_nms takes and nothing else
    dm = _head(PPYOLO_r18vd_Config().nms_cfg).decode_params(outs)
    assert dm['nms_type'] == 'matrix_nms'
    assert dm['nms'] == dict(score_threshold=0.01, post_threshold=0.01, nms_top_k=500, keep_top_k=100, use_gaussian=False,
                             gaussian_sigma=2.)
    assert PPYOLO_r18vd_Config().nms_cfg['nms_type'] == 'matrix_nms'


def test_head_refuses_what_it_does_not_know():
    from config import multiclass_nms_defaults
    outs = [_Out(), _Out()]
    with pytest.raises(NotImplementedError, match='fast_nms'):
        _head(dict(multiclass_nms_defaults(), nms_type='fast_nms')).decode_params(outs)
    with pytest.raises(ValueError, match='post_threshold'):                   # a Matrix-NMS key in a hard-NMS configuration
        _head(dict(multiclass_nms_defaults(), post_threshold=0.01)).decode_params(outs)
    with pytest.raises(ValueError, match='nms_threshold'):                    # and the reverse
        from config import PPYOLO_r18vd_Config
        _head(dict(PPYOLO_r18vd_Config().nms_cfg, nms_threshold=0.45)).decode_params(outs)
    missing = multiclass_nms_defaults()
    del missing['normalized']
    with pytest.raises(ValueError, match='normalized'):
        _head(missing).decode_params(outs)
    for key, val in (('nms_top_k', -1), ('keep_top_k', 0), ('nms_top_k', 1025), ('nms_eta', 0.9)):
        with pytest.raises(ValueError, match=key):
            _head(dict(multiclass_nms_defaults(), **{key: val})).decode_params(outs)
