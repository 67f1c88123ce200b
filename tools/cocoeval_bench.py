"""COCO-val-sized timing of the device COCO evaluator (ppyolo_hip/cocoeval.py).

    python tools/cocoeval_bench.py [--images 5000] [--cats 80] [--gts 8] [--dets 100] [--skew 0.25 --crowded 0.01]
                                   [--reps 5] [--check]

A seeded synthetic set (tests/cocoeval_ref.synthetic: ~36 k GTs, 100 detections per image by default).  By default the
categories are uniform.  --skew gives the first category that share of the GTs and detections (COCO val's `person` holds
about a quarter), and --crowded gives that share of the images 80 extra GTs of it, so that some pairs exceed 64 GTs.
Reports device milliseconds from HIP events for the GT upload, for add() (forward_padded-style rows, batches of 8) and for evaluate()'s
device work, the median of --reps runs.  --check also runs the float64 restatement on the CPU (minutes at full size) and
compares everything bit for bit.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--cats', type=int, default=80)
    ap.add_argument('--gts', type=float, default=8.0)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--skew', type=float, default=0.0)
    ap.add_argument('--crowded', type=float, default=0.0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--check', action='store_true')
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    import cocoeval_ref as R
    from ppyolo_hip.cocoeval import BboxEvaluator, CocoGroundTruth
    t0 = time.time()
    gt, dets = R.synthetic(2024, a.images, a.cats, gt_per_img=a.gts, det_per_img=a.dets, skew=a.skew, crowded=a.crowded)
    gen_s = time.time() - t0
    cat_ids = sorted(c['id'] for c in gt['categories'])
    clsid2catid = {i: c for i, c in enumerate(cat_ids)}
    ev_ms = lambda s, e: s.elapsed_time(e)      # noqa: E731

    # forward_padded-style rows: [N, 100, 6] float32 (label, score, xmin, ymin, xmax, ymax); the writer's inverse so that
    # the records equal the synthetic ones up to the float32 rounding of the rows
    by_img = {}
    for d in dets:
        if d['category_id'] in clsid2catid.values():
            by_img.setdefault(d['image_id'], []).append(d)
    img_ids = [im['id'] for im in gt['images']]
    cls_of = {c: i for i, c in clsid2catid.items()}
    keep_k = max(1, max(len(v) for v in by_img.values()))
    rows = np.full((len(img_ids), keep_k, 6), -1.0, np.float32)
    cnt = np.zeros(len(img_ids), np.int32)
    for j, im in enumerate(img_ids):
        ds = by_img.get(im, [])
        cnt[j] = len(ds)
        for q, d in enumerate(ds):
            x, y, w, h = d['bbox']
            rows[j, q] = [cls_of[d['category_id']], d['score'], x, y, x + w - 1, y + h - 1]
    rows_d = torch.from_numpy(rows).cuda()
    cnt_d = torch.from_numpy(cnt).cuda()

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    up, add, evl = [], [], []
    for _ in range(a.reps + 1):
        g = CocoGroundTruth.from_dict(gt, device='cpu')
        g.device = torch.device('cuda')
        torch.cuda.synchronize()
        s.record()
        g.upload()
        e.record()
        torch.cuda.synchronize()
        up.append(ev_ms(s, e))
        ev = BboxEvaluator(g, clsid2catid=clsid2catid)
        torch.cuda.synchronize()
        s.record()
        for b0 in range(0, len(img_ids), 8):
            ev.add(rows_d[b0:b0 + 8], cnt_d[b0:b0 + 8], img_ids[b0:b0 + 8])
        e.record()
        torch.cuda.synchronize()
        add.append(ev_ms(s, e))
        s.record()
        ev.run()
        e.record()
        torch.cuda.synchronize()
        evl.append(ev_ms(s, e))
    out = ev.evaluate()
    first = sum(1 for x in gt['annotations'] if x['category_id'] == cat_ids[0])
    res = dict(metric='cocoeval_bbox_evaluate_ms', images=len(img_ids), categories=len(cat_ids), gts=len(gt['annotations']),
               first_category_gts=first, largest_pair_gts=g.max_pair_gts,
               records=int(cnt.sum()), gt_upload_ms=float(np.median(up[1:])), add_ms=float(np.median(add[1:])),
               evaluate_ms=float(np.median(evl[1:])), evaluate_ms_all=[round(v, 3) for v in evl[1:]],
               synth_s=round(gen_s, 1), stats=[float(v) for v in out['stats']])
    if a.check:
        rec, pair = ev.records()
        recs = []
        for j in range(len(pair)):
            if pair[j] >= 0:
                recs.append({'image_id': int(g.img_ids[pair[j] // len(cat_ids)]), 'category_id': int(cat_ids[pair[j] % len(cat_ids)]),
                             'bbox': [float(v) for v in rec[j, :4]], 'score': float(rec[j, 5])})
        t0 = time.time()
        p, r, sc = R.evaluate(gt, recs)
        st = R.summarize(p, r)
        res['cpu_restatement_s'] = round(time.time() - t0, 1)
        same = lambda u, v: bool(np.array_equal(np.ascontiguousarray(u).view(np.uint64), np.ascontiguousarray(v).view(np.uint64)))  # noqa: E731
        res['check'] = dict(precision=same(out['precision'], p), recall=same(out['recall'], r), scores=same(out['scores'], sc),
                            stats=same(out['stats'], st))
    print(json.dumps(res))
    if a.check and not all(res['check'].values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
