"""CPU restatement of pycocotools' COCOeval(cocoGt, cocoDt, 'bbox') with default Params -- TEST INFRASTRUCTURE ONLY.

The product (ppyolo_hip/cocoeval.py + csrc/cocoeval.hip) never imports this file.  It restates, loop for loop and in
float64, what COCO.loadRes, COCOeval._prepare / computeIoU / evaluateImg / accumulate / summarize do for bbox results
(maskApi.c bbIou for the IoU).  UNPINNED: pycocotools is not installed in this image, so this restatement is proven on
hand-derived answers (tests/test_cocoeval_ref.py) and the device evaluator is compared against it bit for bit.

gt:   {'images': [{'id'}], 'categories': [{'id'}], 'annotations': [{'id', 'image_id', 'category_id', 'bbox', 'area',
      'iscrowd'}]}   (the annotation file's layout)
dets: [{'image_id', 'category_id', 'bbox': [x, y, w, h], 'score'}]   (the result file's layout)
"""
import math
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def bb_iou(d, g, crowd):
    """maskApi.c bbIou for one (dt, gt) box pair, in double."""
    ga = g[2] * g[3]
    da = d[2] * d[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def load_res(gt, dets):
    """COCO.loadRes for bbox results: ids 1.., area = w * h, iscrowd 0; images outside the GT are an error."""
    img_ids = set(im['id'] for im in gt['images'])
    out = []
    for i, r in enumerate(dets):
        if r['image_id'] not in img_ids:
            raise ValueError('Results do not correspond to current coco set')
        bb = [float(v) for v in r['bbox']]
        if any(math.isnan(v) for v in bb) or math.isnan(float(r['score'])):
            raise ValueError('NaN in a result')
        out.append({'image_id': r['image_id'], 'category_id': r['category_id'], 'bbox': bb, 'score': float(r['score']),
                    'area': bb[2] * bb[3], 'id': i + 1, 'iscrowd': 0})
    return out


def evaluate_img(gt, dt, a_rng, max_det):
    """COCOeval.evaluateImg for one (image, category, area range): gt / dt in order of appearance."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        g['_ignore'] = 1 if (g['ignore'] or (g['area'] < a_rng[0] or g['area'] > a_rng[1])) else 0
    gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(o['iscrowd']) for o in gt]
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gt_ig = np.array([g['_ignore'] for g in gt])
    dt_ig = np.zeros((T, D))
    ious = [[bb_iou(d['bbox'], g['bbox'], iscrowd[gind]) for gind, g in enumerate(gt)] for d in dt]
    for tind, t in enumerate(IOU_THRS):
        for dind, d in enumerate(dt):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind, g in enumerate(gt):
                if gtm[tind, gind] > 0 and not iscrowd[gind]:
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                    break
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = gt_ig[m]
            dtm[tind, dind] = gt[m]['id']
            gtm[tind, m] = d['id']
    a = np.array([d['area'] < a_rng[0] or d['area'] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {'dtMatches': dtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gt_ig, 'dtIgnore': dt_ig}


def evaluate(gt, dets):
    """evaluate() + accumulate() -> (precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M]), all -1 to start."""
    dts = load_res(gt, dets)
    img_ids = sorted(im['id'] for im in gt['images'])
    cat_ids = sorted(c['id'] for c in gt['categories'])
    img_set, cat_set = set(img_ids), set(cat_ids)
    gts_by = defaultdict(list)
    dts_by = defaultdict(list)
    for g in gt['annotations']:
        if g['image_id'] in img_set and g['category_id'] in cat_set:
            g = dict(g)
            g['iscrowd'] = int(g.get('iscrowd', 0))
            g['ignore'] = 1 if g['iscrowd'] else 0
            g['bbox'] = [float(v) for v in g['bbox']]
            g['area'] = float(g['area'])
            gts_by[g['image_id'], g['category_id']].append(g)
    for d in dts:
        if d['category_id'] in cat_set:
            dts_by[d['image_id'], d['category_id']].append(d)
    max_det = MAX_DETS[-1]
    eval_imgs = [evaluate_img(gts_by[i, c], dts_by[i, c], a, max_det)
                 for c in cat_ids for a in AREA_RNG for i in img_ids]
    return accumulate(eval_imgs, len(img_ids), len(cat_ids))


def accumulate(eval_imgs, I0, K0):
    T, R, A0, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K0, A0, M))
    recall = -np.ones((T, K0, A0, M))
    scores = -np.ones((T, R, K0, A0, M))
    for k in range(K0):
        Nk = k * A0 * I0
        for a in range(A0):
            Na = a * I0
            for m, max_det in enumerate(MAX_DETS):
                E = [eval_imgs[Nk + Na + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e['dtScores'][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind='mergesort')
                dt_scores_sorted = dt_scores[inds]
                dtm = np.concatenate([e['dtMatches'][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e['dtIgnore'][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, REC_THRS, side='left')
                    try:
                        for ri, pi in enumerate(inds):
                            q[ri] = pr[pi]
                            ss[ri] = dt_scores_sorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return precision, recall, scores


def summarize(precision, recall, out=None):
    """COCOeval.summarize for bbox: the 12 stats, and pycocotools' 12 lines appended to `out` (a list) if given."""
    def one(ap=1, iou_thr=None, area_rng='all', max_dets=100):
        i_str = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        title = 'Average Precision' if ap == 1 else 'Average Recall'
        typ = '(AP)' if ap == 1 else '(AR)'
        iou_str = '{:0.2f}:{:0.2f}'.format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
        aind = [i for i, r in enumerate(AREA_LBL) if r == area_rng]
        mind = [i for i, d in enumerate(MAX_DETS) if d == max_dets]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        if out is not None:
            out.append(i_str.format(title, typ, iou_str, area_rng, max_dets, mean_s))
        return mean_s
    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iou_thr=.5, max_dets=MAX_DETS[2])
    stats[2] = one(1, iou_thr=.75, max_dets=MAX_DETS[2])
    stats[3] = one(1, area_rng='small', max_dets=MAX_DETS[2])
    stats[4] = one(1, area_rng='medium', max_dets=MAX_DETS[2])
    stats[5] = one(1, area_rng='large', max_dets=MAX_DETS[2])
    stats[6] = one(0, max_dets=MAX_DETS[0])
    stats[7] = one(0, max_dets=MAX_DETS[1])
    stats[8] = one(0, max_dets=MAX_DETS[2])
    stats[9] = one(0, area_rng='small', max_dets=MAX_DETS[2])
    stats[10] = one(0, area_rng='medium', max_dets=MAX_DETS[2])
    stats[11] = one(0, area_rng='large', max_dets=MAX_DETS[2])
    return stats


def synthetic(seed, n_img, n_cat, gt_per_img=7.2, det_per_img=100, pair_dets=None, crowd=0.02, no_gt_frac=0.1, levels=40,
              skew=0.0, crowded=0.0):
    """A seeded COCO-like (gt, dets): non-contiguous image / category ids, ~2 % crowd, boxes and `area` fields on and near
    the small / medium bounds, images without GTs, scores on a coarse grid (ties), detections jittered from GTs or random,
    a few on a category outside the GT, bboxes rounded to 0.1 as the result writer does.  pair_dets=(lo, hi): instead of
    det_per_img random detections per image, lo..hi detections for each of 1-3 categories of every image.  skew: the share
    of GTs and random detections that go to the first category (COCO's `person` holds about a quarter); crowded: the share
    of images that also get 80 GTs of the first category (pairs beyond 64 GTs)."""

    def pick_cat():
        if skew > 0 and rng.rand() < skew:
            return cat_ids[0]
        return cat_ids[rng.randint(n_cat)]
    rng = np.random.RandomState(seed)
    img_ids = [int(v) + 1 for v in rng.choice(10 ** 6, n_img, replace=False)]
    cat_ids = sorted(int(v) + 1 for v in rng.choice(10 * n_cat, n_cat, replace=False))
    anns = []
    per_img = {}
    for j, im in enumerate(img_ids):
        n = 0 if j < int(no_gt_frac * n_img) else rng.poisson(gt_per_img)
        per_img[im] = []
        for _ in range(n):
            kind = rng.randint(4)
            if kind == 0:
                w = h = float(rng.choice([32.0, 96.0]))
            elif kind == 1:
                w, h = round(float(rng.choice([32, 96]) + rng.uniform(-0.3, 0.3)), 2), float(rng.choice([32, 96]))
            else:
                w, h = round(float(rng.uniform(2, 300)), 2), round(float(rng.uniform(2, 300)), 2)
            x, y = round(float(rng.uniform(0, 600)), 2), round(float(rng.uniform(0, 600)), 2)
            area = w * h if rng.rand() < 0.9 else float(rng.choice([1024.0, 9216.0, w * h * 0.9]))
            c = pick_cat()
            a = {'id': len(anns) + 1, 'image_id': im, 'category_id': c, 'bbox': [x, y, w, h], 'area': area,
                 'iscrowd': int(rng.rand() < crowd)}
            anns.append(a)
            per_img[im].append(a)
        if crowded > 0 and j >= int(no_gt_frac * n_img) and rng.rand() < crowded:
            for _ in range(80):
                x, y = round(float(rng.uniform(0, 600)), 2), round(float(rng.uniform(0, 600)), 2)
                w, h = round(float(rng.uniform(8, 60)), 2), round(float(rng.uniform(8, 60)), 2)
                a = {'id': len(anns) + 1, 'image_id': im, 'category_id': cat_ids[0], 'bbox': [x, y, w, h], 'area': w * h,
                     'iscrowd': 0}
                anns.append(a)
                per_img[im].append(a)
    gt = {'images': [{'id': im} for im in img_ids], 'categories': [{'id': c} for c in cat_ids], 'annotations': anns}

    def one_det(im, c):
        src = per_img[im]
        if src and rng.rand() < 0.6:
            g = src[rng.randint(len(src))]
            x, y, w, h = g['bbox']
            j = rng.uniform(-0.25, 0.25, 4) * np.array([w, h, w, h]) * rng.choice([0.0, 0.2, 1.0])
            box = [x + j[0], y + j[1], max(w + j[2], 0.5), max(h + j[3], 0.5)]
            if c is None:
                c = g['category_id'] if rng.rand() < 0.8 else pick_cat()
        else:
            box = [rng.uniform(0, 600), rng.uniform(0, 600), rng.uniform(1, 200), rng.uniform(1, 200)]
            if c is None:
                c = pick_cat() if rng.rand() < 0.99 else 10 ** 6
        return {'image_id': im, 'category_id': c, 'bbox': [round(float(v) * 10) / 10 for v in box],
                'score': float(rng.randint(1, levels + 1)) / levels}
    dets = []
    for im in img_ids:
        if pair_dets is None:
            dets += [one_det(im, None) for _ in range(det_per_img)]
        else:
            for c in rng.choice(cat_ids, rng.randint(1, 4), replace=False):
                dets += [one_det(im, int(c)) for _ in range(rng.randint(pair_dets[0], pair_dets[1] + 1))]
    return gt, dets
