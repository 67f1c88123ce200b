"""The device COCO evaluator (ppyolo_hip/cocoeval.py + csrc/cocoeval.hip) against the float64 restatement
(tests/cocoeval_ref.py), bit for bit: precision, recall, scores and the 12 stats.  The record arithmetic is pinned to JSON
the reference itself wrote (g10); the end-to-end case scores the model's detections on g18's input."""
import json
import os

import numpy as np
import pytest
import torch

import cocoeval_ref as R
from test_cocoeval_ref import CASES

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _device(gt, dets, iou_row_gts=None):
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    ev = BboxEvaluator(CocoGroundTruth.from_dict(gt))
    if iou_row_gts is not None:
        ev.iou_row_gts = iou_row_gts
    ev.add_records(dets)
    return ev, ev.evaluate()


def _check(gt, dets, out):
    p, r, s = R.evaluate(gt, dets)
    st = R.summarize(p, r)
    assert _bits_equal(out['precision'], p), np.argwhere(out['precision'] != p)[:5]
    assert _bits_equal(out['recall'], r), np.argwhere(out['recall'] != r)[:5]
    assert _bits_equal(out['scores'], s), np.argwhere(out['scores'] != s)[:5]
    assert _bits_equal(out['stats'], st), (out['stats'], st)
    return st


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_cases(name):
    gt, dets = CASES[name]()
    ev, out = _device(gt, dets)
    _check(gt, dets, out)


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_random_small_sets(seed):
    gt, dets = R.synthetic(100 + seed, 10 + 13 * seed, 3 + 2 * seed, gt_per_img=4 + 3 * seed, pair_dets=(0, 150))
    ev, out = _device(gt, dets)
    _check(gt, dets, out)


@pytest.mark.parametrize('row', [None, 0, 40])
def test_many_gts_in_a_pair(row):
    """90 GTs in one pair, 120 detections: the IoU row in LDS (row None: sized to the largest pair), and pairs beyond the
    row recomputing their IoUs in every chain (row 0: all pairs; row 40: the big pair only)."""
    rng = np.random.RandomState(7)
    anns = [{'id': j + 1, 'image_id': 1, 'category_id': 1, 'bbox': [float(v) for v in np.round(rng.uniform(0, 80, 4), 1)],
             'area': 0.0, 'iscrowd': int(j % 17 == 0)} for j in range(90)]
    for a in anns:
        a['bbox'][2] += 5
        a['bbox'][3] += 5
        a['area'] = a['bbox'][2] * a['bbox'][3]
    gt = {'images': [{'id': 1}, {'id': 2}], 'categories': [{'id': 1}], 'annotations': anns}
    dets = [{'image_id': 1, 'category_id': 1, 'bbox': [round(float(v), 1) for v in rng.uniform(0, 80, 2)] + [30.0, 30.0],
             'score': float(rng.randint(20)) / 20} for _ in range(120)]
    dets += [{'image_id': 2, 'category_id': 1, 'bbox': [1.0, 1.0, 9.0, 9.0], 'score': .5}]
    ev, out = _device(gt, dets, row)
    _check(gt, dets, out)


def test_recompute_path_on_a_random_set():
    gt, dets = R.synthetic(21, 30, 4, gt_per_img=9, pair_dets=(0, 120))
    ev, out = _device(gt, dets, 1)
    _check(gt, dets, out)


def test_random_medium_set_and_repeatable():
    gt, dets = R.synthetic(11, 500, 80, det_per_img=100)
    ev, out = _device(gt, dets)
    st = _check(gt, dets, out)
    again = ev.evaluate()
    for k in ('precision', 'recall', 'scores', 'stats'):
        assert _bits_equal(again[k], out[k])
    assert st[0] > 0.05


def _pad_rows(boxes, scores, classes, keep_k):
    rows = np.full((keep_k, 6), -1.0, dtype=np.float32)
    k = len(scores)
    if k:
        rows[:k, 0] = classes
        rows[:k, 1] = scores
        rows[:k, 2:] = boxes
    return rows, k


def test_record_arithmetic_equals_reference_json(golden):
    """dets rows -> device records: the doubles the reference's writer put in its JSON (g10), exactly."""
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    from tools import cocotools
    g = golden('g10_coco_records')
    n = int(g['ncases'])
    cases = []
    for j in range(n):
        b, s, c = g['boxes%d' % j], g['scores%d' % j], g['classes%d' % j]
        if b.size == 0:
            b, s, c = np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)
        cases.append((b.astype(np.float32), s.astype(np.float32), c, int(g['im_id%d' % j]), json.loads(bytes(g['json%d' % j]).decode())))
    gt = {'images': [{'id': c[3]} for c in cases], 'categories': [{'id': v} for v in cocotools.clsid2catid.values()],
          'annotations': []}
    ev = BboxEvaluator(CocoGroundTruth.from_dict(gt), clsid2catid=cocotools.clsid2catid)
    rows, cnt = zip(*[_pad_rows(c[0], c[1], c[2], 100) for c in cases])
    ev.add(torch.from_numpy(np.stack(rows)).cuda(), torch.tensor(cnt, dtype=torch.int32).cuda(), [c[3] for c in cases])
    rec, pair = ev.records()
    cat_ids = ev.gt.cat_ids
    total = 0
    for j, c in enumerate(cases):
        want = c[4]
        assert (pair[j * 100:(j + 1) * 100] >= 0).sum() == len(want)
        for q, w in enumerate(want):
            r = rec[j * 100 + q]
            assert list(r[:4]) == w['bbox'] and r[5] == w['score'] and r[4] == w['bbox'][2] * w['bbox'][3]
            assert cat_ids[pair[j * 100 + q] % len(cat_ids)] == w['category_id']
            total += 1
    assert total > 100


def test_add_path_equals_writer_then_bbox_eval(tmp_path, monkeypatch, capsys):
    """forward_padded-style tensors through add() == the same detections through write_batch + bbox_eval (the reference's
    file path), including images with count 0; and == the restatement."""
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    from tools import cocotools
    gt, _ = R.synthetic(5, 24, 80, gt_per_img=6)
    cat_of = {i: c for i, c in cocotools.clsid2catid.items()}
    gt['categories'] = [{'id': c} for c in sorted(cat_of.values())]
    cats = sorted(cat_of.values())
    clsid = {c: i for i, c in cat_of.items()}
    for a in gt['annotations']:
        a['category_id'] = cats[hash((a['id'], 3)) % len(cats)]
    anno = tmp_path / 'anno.json'
    anno.write_text(json.dumps(gt))
    rng = np.random.RandomState(3)
    img_ids = [im['id'] for im in gt['images']]
    keep_k = 100
    batches = []
    for b0 in range(0, len(img_ids), 8):
        ids = img_ids[b0:b0 + 8]
        rows, cnt = [], []
        for j, im in enumerate(ids):
            k = 0 if j % 5 == 2 else int(rng.randint(1, keep_k + 1))
            src = [a for a in gt['annotations'] if a['image_id'] == im]
            boxes = np.zeros((k, 4), np.float32)
            cls = np.zeros(k, np.int32)
            for q in range(k):
                if src and rng.rand() < 0.6:
                    a = src[rng.randint(len(src))]
                    x, y, w, h = a['bbox']
                    boxes[q] = [x, y, x + w - 1, y + h - 1] + rng.uniform(-2, 2, 4)
                    cls[q] = clsid[a['category_id']]
                else:
                    x, y = rng.uniform(0, 500, 2)
                    boxes[q] = [x, y, x + rng.uniform(1, 150), y + rng.uniform(1, 150)]
                    cls[q] = rng.randint(80)
            scores = (rng.randint(1, 30, k) / 30).astype(np.float32)
            r, n = _pad_rows(boxes, scores, cls, keep_k)
            rows.append(r)
            cnt.append(n)
        batches.append((ids, np.stack(rows), np.array(cnt, np.int32)))
    ev = BboxEvaluator(CocoGroundTruth.from_json(str(anno)), clsid2catid=cocotools.clsid2catid)
    dev_rows = torch.empty((8, keep_k, 6), dtype=torch.float32, device='cuda')
    for ids, rows, cnt in batches:
        dev_rows[:len(ids)].copy_(torch.from_numpy(rows))
        ev.add(dev_rows[:len(ids)], torch.from_numpy(cnt).cuda(), ids)
        dev_rows.fill_(-7.0)                      # the next forward overwrites the rows: add() must have copied them
    out = ev.evaluate()
    monkeypatch.chdir(tmp_path)
    os.makedirs('eval_results/bbox')
    for ids, rows, cnt in batches:
        cocotools.write_batch('eval_results', [rows[j, :cnt[j], 2:] for j in range(len(ids))],
                              [rows[j, :cnt[j], 1] for j in range(len(ids))], [rows[j, :cnt[j], 0].astype(np.int32) for j in range(len(ids))],
                              ids, ['%d.jpg' % i for i in ids])
    stats = cocotools.bbox_eval(str(anno))
    printed = capsys.readouterr().out
    assert 'Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]' in printed
    assert _bits_equal(stats, out['stats'])
    recs = json.load(open('eval_results/bbox_detections.json'))
    assert sum(1 for _ in recs) == int(sum(c.sum() for _, _, c in batches))
    _check(gt, recs, out)


def test_end_to_end_r50vd_608(golden):
    """R50vd-608 bs 8 forward_padded on g18's input, scored against GTs made from the reference's own rows for that input
    (the writer's convention: area = w * h, iscrowd 0): bit-equal to the restatement, and AP >= 0.99."""
    from conftest import build_model
    from config import PPYOLO_2x_Config
    from ppyolo_hip import synth
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    from tools import cocotools
    g = golden('g18_r50vd_608')
    S, N = int(g['meta'][0]), int(g['meta'][1])
    img_ids = [1000 + 7 * i for i in range(N)]
    anns = []
    for i in range(N):
        ref = g['t8_a_pred%d' % i]
        for r in cocotools.bbox_records(ref[:, 2:], ref[:, 1], ref[:, 0].astype(np.int32), img_ids[i]):
            anns.append({'id': len(anns) + 1, 'image_id': r['image_id'], 'category_id': r['category_id'], 'bbox': r['bbox'],
                         'area': r['bbox'][2] * r['bbox'][3], 'iscrowd': 0})
    gt = {'images': [{'id': i} for i in img_ids], 'categories': [{'id': c} for c in cocotools.clsid2catid.values()],
          'annotations': anns}
    model, _ = build_model(PPYOLO_2x_Config(), 0, 'cuda')
    x = synth.synth_images(N, S).cuda()
    dets, cnt, _ = model.forward_padded(x, torch.from_numpy(g['im_size_a']).cuda())
    ev = BboxEvaluator(CocoGroundTruth.from_dict(gt), clsid2catid=cocotools.clsid2catid)
    ev.add(dets, cnt, img_ids)
    out = ev.evaluate()
    d, c = dets.cpu().numpy(), cnt.cpu().numpy()
    recs = []
    for i in range(N):
        k = int(c[i])
        recs += cocotools.bbox_records(d[i, :k, 2:], d[i, :k, 1], d[i, :k, 0].astype(np.int32), img_ids[i])
    st = _check(gt, recs, out)
    assert np.all(st[0:3] >= 0.99), st


def _one_image_gt():
    from tools import cocotools
    anns = [{'id': 1, 'image_id': 5, 'category_id': cocotools.clsid2catid[0], 'bbox': [10.0, 10.0, 50.0, 40.0], 'area': 2000.0,
             'iscrowd': 0}]
    # category 1's id is left out of the GT: rows of model class 1 are not records
    cats = [c for i, c in cocotools.clsid2catid.items() if i != 1]
    return {'images': [{'id': 5}, {'id': 6}], 'categories': [{'id': c} for c in cats], 'annotations': anns}


def test_rows_of_classes_outside_the_gt_are_dropped():
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    from tools import cocotools
    gt = _one_image_gt()
    rows = np.full((2, 4, 6), -1.0, np.float32)
    rows[0, 0] = [0, .9, 10, 10, 59, 49]            # class 0: a TP
    rows[0, 1] = [1, .95, 10, 10, 59, 49]           # class 1: its category is not in the GT
    rows[0, 2] = [200, .97, 10, 10, 59, 49]         # a class beyond the table
    rows[1, 0] = [0, .8, 300, 300, 320, 330]        # image 6: an FP
    ev = BboxEvaluator(CocoGroundTruth.from_dict(gt), clsid2catid=cocotools.clsid2catid)
    ev.add(torch.from_numpy(rows).cuda(), torch.tensor([3, 1], dtype=torch.int32).cuda(), [5, 6])
    rec, pair = ev.records()
    assert pair.tolist() == [0 * 79 + 0, -1, -1, -1, 1 * 79 + 0, -1, -1, -1]
    out = ev.evaluate()
    recs = cocotools.bbox_records(rows[0, :1, 2:], rows[0, :1, 1], [0], 5) + cocotools.bbox_records(rows[1, :1, 2:], rows[1, :1, 1], [0], 6)
    _check(gt, recs, out)
    assert out['stats'][0] > 0.5


def test_nan_row_makes_evaluate_raise():
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    from tools import cocotools
    ev = BboxEvaluator(CocoGroundTruth.from_dict(_one_image_gt()), clsid2catid=cocotools.clsid2catid)
    rows = np.full((1, 4, 6), -1.0, np.float32)
    rows[0, 0] = [0, .9, 10, 10, 59, 49]
    rows[0, 1] = [0, .5, 10, float('nan'), 59, 49]
    rows[0, 2] = [0, float('nan'), 10, 10, 59, 49]  # beyond count: not a record, never inspected
    ev.add(torch.from_numpy(rows).cuda(), torch.tensor([2], dtype=torch.int32).cuda(), [5])
    with pytest.raises(ValueError, match='NaN'):
        ev.evaluate()
    ev.reset()
    ev.add(torch.from_numpy(rows).cuda(), torch.tensor([1], dtype=torch.int32).cuda(), [5])
    assert ev.evaluate()['stats'][0] == 1.0 / (1.0 + np.spacing(1))
