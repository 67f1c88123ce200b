"""Host side of the COCO evaluator (no GPU): GT grouping, result-record parsing, and the reference's tools/cocotools.py
names (get_classes / cocoapi_eval / bbox_eval, reference tools/cocotools.py:40-98) with its exact parameter lists."""
import inspect

import numpy as np
import pytest

from ppyolo_hip import cocoeval as C


def _gt():
    return {'images': [{'id': 30}, {'id': 10}, {'id': 20}], 'categories': [{'id': 5}, {'id': 2}],
            'annotations': [
                {'id': 1, 'image_id': 20, 'category_id': 5, 'bbox': [0, 0, 4, 4], 'area': 16, 'iscrowd': 0},
                {'id': 2, 'image_id': 10, 'category_id': 2, 'bbox': [1, 1, 2, 2], 'area': 4, 'iscrowd': 1},
                {'id': 3, 'image_id': 20, 'category_id': 5, 'bbox': [2, 2, 4, 4], 'area': 15.5},
                {'id': 4, 'image_id': 99, 'category_id': 5, 'bbox': [2, 2, 4, 4], 'area': 16, 'iscrowd': 0},
                {'id': 0, 'image_id': 20, 'category_id': 2, 'bbox': [3, 3, 1, 1], 'area': 1, 'iscrowd': 0},
                {'id': 6, 'image_id': 20, 'category_id': 7, 'bbox': [3, 3, 1, 1], 'area': 1, 'iscrowd': 0},
                {'id': 7, 'image_id': 20, 'category_id': 5, 'bbox': [9, 9, 1, 1], 'area': 1, 'iscrowd': 0}]}


def test_gt_grouping_and_order():
    g = C.CocoGroundTruth.from_dict(_gt(), device='cpu')
    assert g.img_ids.tolist() == [10, 20, 30] and g.cat_ids.tolist() == [2, 5]
    # pairs (image index * K + category index), GTs of a pair in file order; unknown image / category dropped
    assert g.pair.tolist() == [0, 2, 3, 3, 3] and g.ids.tolist() == [2, 0, 1, 3, 7]
    assert g.off.tolist() == [0, 1, 1, 2, 5, 5, 5] and g.cat_off.tolist() == [0, 2, 5]
    assert g.crowd.tolist() == [1, 0, 0, 0, 0] and g.area.tolist() == [4, 1, 16, 15.5, 1]
    assert g.box[3].tolist() == [2, 2, 4, 4]
    assert g.d_idnz.tolist() == [1, 0, 1, 1, 1] and g.d_off.dtype.is_floating_point is False


def test_record_parsing():
    g = C.CocoGroundTruth.from_dict(_gt(), device='cpu')
    recs = [{'image_id': 30, 'category_id': 5, 'bbox': [1.5, 2, 3.1, 4.2], 'score': 0.25},
            {'image_id': 10, 'category_id': 8, 'bbox': [0, 0, 1, 1], 'score': 0.5},
            {'image_id': 20, 'category_id': 2, 'bbox': [0, 0, 1, 1], 'score': 1}]
    rec, pair = C.records_to_arrays(g, recs)
    assert rec[0].tolist() == [1.5, 2.0, 3.1, 4.2, 3.1 * 4.2, 0.25]
    assert pair.tolist() == [2 * 2 + 1, -1, 1 * 2 + 0]
    with pytest.raises(ValueError):
        C.records_to_arrays(g, [{'image_id': 11, 'category_id': 5, 'bbox': [0, 0, 1, 1], 'score': .5}])
    with pytest.raises(ValueError):
        C.records_to_arrays(g, [{'image_id': 10, 'category_id': 5, 'bbox': [0, 0, 1, 1], 'score': float('nan')}])


def test_params_are_numpys():
    assert np.array_equal(C.IOU_THRS, np.linspace(.5, .95, 10)) and np.array_equal(C.REC_THRS, np.linspace(0, 1, 101))
    assert C.AREA_RNG == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]] and C.MAX_DETS == [1, 10, 100]


def test_summarize_stats_empty_and_lines():
    p = -np.ones((10, 101, 2, 4, 3))
    r = -np.ones((10, 2, 4, 3))
    lines = []
    st = C.summarize_stats(p, r, lines)
    assert np.all(st == -1) and len(lines) == 12
    assert lines[11] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000'


def test_cocotools_has_the_reference_eval_api(tmp_path):
    from tools import cocotools
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    E = inspect.Parameter.empty
    assert sig(cocotools.get_classes) == [('classes_path', E)]
    assert sig(cocotools.cocoapi_eval) == [('jsonfile', E), ('style', E), ('coco_gt', None), ('anno_file', None),
                                           ('max_dets', (100, 300, 1000))]
    assert sig(cocotools.bbox_eval) == [('anno_file', E)]
    f = tmp_path / 'classes.txt'
    f.write_text('person\n bicycle \ncar\n')
    assert cocotools.get_classes(str(f)) == ['person', 'bicycle', 'car']
    with pytest.raises(NotImplementedError):
        cocotools.cocoapi_eval('x.json', 'segm', anno_file='a.json')
