"""COCO result records -- the on-disk format on the far side of the path: what the
reference's eval / test-dev harness writes per image after `Decode.detect_batch` (reference tools/cocotools.py:159-191,
called from :230-247).  Same import name (`from tools.cocotools import ...`), same record layout and rounding:

    {'image_id': id, 'category_id': clsid2catid[class], 'bbox': [xmin, ymin, w, h], 'score': float(score)}
    w = xmax - xmin + 1, h = ymax - ymin + 1        (computed in the dtype of the box array, float32)
    every bbox entry -> round(float(v) * 10) / 10   (Python round: half to even, on the float64 product)

one JSON list per image in `<result_dir>/bbox/<image name without extension>.json`.  The mAP computation the reference
runs on these files (:44-98, pycocotools COCOeval) is here under the same names -- get_classes, cocoapi_eval, bbox_eval --
on top of ppyolo_hip.cocoeval, which evaluates on the device with COCOeval's semantics (bbox style only).  Drawing (cv2) is
not provided.
"""
import glob
import json
import logging
import os

logger = logging.getLogger(__name__)

# contiguous class index -> COCO category id: the ids 1..90 without the ten ids COCO never used
# (the reference spells the table out, tools/cocotools.py:22-38)
_UNUSED_CATIDS = (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)
clsid2catid = {i: c for i, c in enumerate(c for c in range(1, 91) if c not in _UNUSED_CATIDS)}
catid2clsid = {c: i for i, c in clsid2catid.items()}


def bbox_records(boxes, scores, classes, im_id, _clsid2catid=None):
    """Records of one image from the arrays `Decode.detect_image / detect_batch` return (boxes [K,4] xyxy, scores [K],
    classes [K]); reference tools/cocotools.py:168-186."""
    m = clsid2catid if _clsid2catid is None else _clsid2catid
    out = []
    for p in range(len(boxes)):
        xmin, ymin, xmax, ymax = boxes[p]
        w = xmax - xmin + 1
        h = ymax - ymin + 1
        out.append({'image_id': im_id, 'category_id': m[int(classes[p])],
                    'bbox': [round(float(v) * 10) / 10 for v in (xmin, ymin, w, h)], 'score': float(scores[p])})
    return out


def write_bbox_json(result_dir, im_name, boxes, scores, classes, im_id, _clsid2catid=None):
    """One image -> `<result_dir>/bbox/<stem>.json` (reference :187-191).  `boxes is None` (the reference's marker for an
    image without detections in its result lists) writes nothing, like the reference."""
    if boxes is None:
        return None
    path = '%s/bbox/%s.json' % (result_dir, im_name.split('.')[0])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(bbox_records(boxes, scores, classes, im_id, _clsid2catid), f)
    return path


def write_batch(result_dir, result_boxes, result_scores, result_classes, batch_im_id, batch_im_name, _clsid2catid=None):
    """The per-batch loop of the reference's eval (tools/cocotools.py:236-247; its writer threads are an implementation
    detail): `Decode.detect_batch` results -> one file per image.  An image whose detection arrays are empty (this
    build's and the reference's `detect_batch` return three empty arrays for it) gets an empty list, which is what the
    reference writes for `len(boxes) == 0`."""
    paths = []
    for j in range(len(result_boxes)):
        paths.append(write_bbox_json(result_dir, batch_im_name[j], result_boxes[j], result_scores[j], result_classes[j],
                                     batch_im_id[j], _clsid2catid))
    return paths


def get_classes(classes_path):
    """Names listed in a text file, one per line, surrounding whitespace removed (reference tools/cocotools.py:38-42)."""
    with open(classes_path) as fh:
        return [line.strip() for line in fh]


def cocoapi_eval(jsonfile, style, coco_gt=None, anno_file=None, max_dets=(100, 300, 1000)):
    """COCOeval of the result file `jsonfile` against `coco_gt` (a ppyolo_hip.cocoeval.CocoGroundTruth) or the annotation
    file `anno_file`; prints the 12 summary lines and returns the 12 stats (reference :44-73).  Only style 'bbox' exists
    here; as in the reference, `max_dets` is read by the 'proposal' style only, so 'bbox' ignores it."""
    if coco_gt is None and anno_file is None:
        raise ValueError('cocoapi_eval needs coco_gt or anno_file')
    if style != 'bbox':
        raise NotImplementedError("cocoapi_eval: only style 'bbox' is provided (got %r)" % (style,))
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    gt = coco_gt if coco_gt is not None else CocoGroundTruth.from_json(anno_file)
    logger.info('COCO bbox evaluation of %s on the device', jsonfile)
    evaluator = BboxEvaluator(gt)
    with open(jsonfile) as fh:
        evaluator.add_records(json.load(fh))
    evaluator.evaluate()
    return evaluator.summarize()


RESULT_DIR = 'eval_results'


def bbox_eval(anno_file):
    """The file side of the reference's eval (:75-98): the per-image lists in `eval_results/bbox/*.json` are merged into
    one list, written to `eval_results/bbox_detections.json`, and scored with cocoapi_eval; returns the 12 stats.  The
    order of the files does not change the result (each holds the records of one image)."""
    from ppyolo_hip.cocoeval import CocoGroundTruth
    gt = CocoGroundTruth.from_json(anno_file)
    merged = []
    for path in sorted(glob.glob(os.path.join(RESULT_DIR, 'bbox', '*.json'))):
        with open(path, encoding='utf-8') as fh:
            merged.extend(json.load(fh))
    merged_path = os.path.join(RESULT_DIR, 'bbox_detections.json')
    logger.info('%d records from %s/bbox -> %s', len(merged), RESULT_DIR, merged_path)
    with open(merged_path, 'w') as fh:
        json.dump(merged, fh)
    return cocoapi_eval(merged_path, 'bbox', coco_gt=gt)
