"""COCO bbox mAP on the device: pycocotools COCOeval(cocoGt, cocoDt, 'bbox') with its default Params -- evaluate(),
accumulate(), summarize() -- bit for bit in float64 (csrc/cocoeval.hip).  The reference ends its eval
in tools/cocotools.py:44-98 (bbox_eval -> cocoapi_eval -> COCOeval); tools/cocotools.py here keeps those names on top of
this module.

    gt = CocoGroundTruth.from_json('annotations/instances_val2017.json')     # parsed and uploaded once
    ev = BboxEvaluator(gt, clsid2catid=clsid2catid)
    for x, im_size, im_ids in loader:
        dets, count, _ = model.forward_padded(x, im_size)
        ev.add(dets, count, im_ids)                                           # no host sync; the rows are copied
    ev.evaluate()['stats']; ev.summarize()

The JSON path (`add_records`) takes the result records the reference writes.  Nothing here computes with torch ops: torch
holds the device memory, the kernels do the work, and the host only parses, groups the GTs once and forms the 12 means.
"""
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib

# pycocotools Params.setDetParams
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def _stream():
    return torch.cuda.current_stream().cuda_stream


class CocoGroundTruth(object):
    """The annotation file, grouped per (image, category) pair on the host and uploaded once.  Images and categories are
    indexed in sorted id order (COCOeval's imgIds / catIds); GTs of a pair keep their order in the file.  Annotations on
    images or categories the file does not list are dropped, as COCOeval's getAnnIds(imgIds, catIds) drops them."""

    def __init__(self, dataset, device='cuda'):
        self.img_ids = np.array(sorted(int(im['id']) for im in dataset['images']), dtype=np.int64)
        self.cat_ids = np.array(sorted(int(c['id']) for c in dataset['categories']), dtype=np.int64)
        if len(self.img_ids) == 0 or len(self.cat_ids) == 0:
            raise ValueError('the ground truth needs at least one image and one category')
        self.img_index = {int(v): i for i, v in enumerate(self.img_ids)}
        self.cat_index = {int(v): k for k, v in enumerate(self.cat_ids)}
        I, K = len(self.img_ids), len(self.cat_ids)
        pair, box, area, crowd, ids = [], [], [], [], []
        for a in dataset['annotations']:
            i, k = self.img_index.get(int(a['image_id'])), self.cat_index.get(int(a['category_id']))
            if i is None or k is None:
                continue
            pair.append(i * K + k)
            box.append([float(v) for v in a['bbox']])
            area.append(float(a['area']))
            crowd.append(1 if a.get('iscrowd', 0) else 0)
            ids.append(int(a['id']))
        pair = np.array(pair, dtype=np.int64)
        order = np.argsort(pair, kind='stable')
        self.pair = pair[order]
        self.box = np.array(box, dtype=np.float64).reshape(-1, 4)[order]
        self.area = np.array(area, dtype=np.float64)[order]
        self.crowd = np.array(crowd, dtype=np.int32)[order]
        self.ids = np.array(ids, dtype=np.int64)[order]
        self.off = np.zeros(I * K + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.pair, minlength=I * K), out=self.off[1:])
        self.cat_off = np.zeros(K + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.pair % K, minlength=K), out=self.cat_off[1:])
        self.num_images, self.num_cats, self.num_gts = I, K, len(self.pair)
        self.max_pair_gts = int(np.diff(self.off).max()) if len(self.pair) else 0
        if I * K >= 2 ** 31 - 1 or self.num_gts >= 2 ** 31 - 1:
            raise ValueError('too many (image, category) pairs or GTs')
        self.device = torch.device(device)
        self.upload()

    def upload(self):
        """Host arrays -> device (the one-time cost the bench reports apart from evaluate)."""
        dev = self.device
        self.d_off = torch.from_numpy(self.off.astype(np.int32)).to(dev)
        self.d_box = torch.from_numpy(np.ascontiguousarray(self.box)).to(dev)
        self.d_area = torch.from_numpy(self.area).to(dev)
        self.d_crowd = torch.from_numpy(self.crowd).to(dev)
        self.d_idnz = torch.from_numpy((self.ids != 0).astype(np.int32)).to(dev)
        self.d_cat_off = torch.from_numpy(self.cat_off.astype(np.int32)).to(dev)

    @classmethod
    def from_dict(cls, dataset, device='cuda'):
        return cls(dataset, device)

    @classmethod
    def from_json(cls, anno_file, device='cuda'):
        with open(anno_file, 'r') as f:
            return cls(json.load(f), device)


def records_to_arrays(gt, records):
    """Result records (COCO.loadRes input) -> (rec [n, 6] float64 = x, y, w, h, area = w * h, score; pair [n] int32, -1 for a
    category outside the GT).  A record on an image outside the GT raises, as loadRes' assert does; so does a NaN."""
    n = len(records)
    rec = np.empty((n, 6), dtype=np.float64)
    pair = np.empty(n, dtype=np.int32)
    K = gt.num_cats
    for j, r in enumerate(records):
        i = gt.img_index.get(int(r['image_id']))
        if i is None:
            raise ValueError('Results do not correspond to current coco set: image_id %r' % (r['image_id'],))
        bb = r['bbox']
        x, y, w, h, s = float(bb[0]), float(bb[1]), float(bb[2]), float(bb[3]), float(r['score'])
        if math.isnan(x) or math.isnan(y) or math.isnan(w) or math.isnan(h) or math.isnan(s):
            raise ValueError('NaN in result record %d' % j)
        rec[j] = (x, y, w, h, w * h, s)
        k = gt.cat_index.get(int(r['category_id']))
        pair[j] = -1 if k is None else i * K + k
    return rec, pair


def summarize_stats(precision, recall, lines=None):
    """COCOeval.summarize() for bbox on the accumulated arrays: the 12 stats (np.mean(s[s > -1]) per line) and, if `lines`
    is a list, pycocotools' 12 lines appended to it."""
    def one(ap=1, iou_thr=None, area_rng='all', max_dets=100):
        i_str = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        title = 'Average Precision' if ap == 1 else 'Average Recall'
        typ = '(AP)' if ap == 1 else '(AR)'
        iou_str = '{:0.2f}:{:0.2f}'.format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
        aind = [i for i, r in enumerate(AREA_LBL) if r == area_rng]
        mind = [i for i, d in enumerate(MAX_DETS) if d == max_dets]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        if lines is not None:
            lines.append(i_str.format(title, typ, iou_str, area_rng, max_dets, mean_s))
        return mean_s
    m = MAX_DETS
    spec = [(1, None, 'all', m[2]), (1, .5, 'all', m[2]), (1, .75, 'all', m[2]), (1, None, 'small', m[2]),
            (1, None, 'medium', m[2]), (1, None, 'large', m[2]), (0, None, 'all', m[0]), (0, None, 'all', m[1]),
            (0, None, 'all', m[2]), (0, None, 'small', m[2]), (0, None, 'medium', m[2]), (0, None, 'large', m[2])]
    stats = np.zeros((12,))
    for j, (ap, thr, rng, md) in enumerate(spec):
        stats[j] = one(ap, thr, rng, md)
    return stats


class BboxEvaluator(object):
    """Detections of a whole eval run, kept on the device, scored against `gt` (a CocoGroundTruth).  clsid2catid maps the
    model's class index to a category id (default: the COCO 80-class table of tools/cocotools.py)."""

    def __init__(self, gt, clsid2catid=None):
        if clsid2catid is None:
            from tools.cocotools import clsid2catid
        self.gt = gt
        dev = gt.device
        self.device = dev
        ncls = max(int(c) for c in clsid2catid) + 1
        lut = np.full(ncls, -1, dtype=np.int32)
        for c, cat in clsid2catid.items():
            lut[int(c)] = gt.cat_index.get(int(cat), -1)
        self._cls2k = torch.from_numpy(lut).to(dev)
        self._ncls = ncls
        self._iou = torch.from_numpy(IOU_THRS.astype(np.float64)).to(dev)          # numpy's doubles, never recomputed
        self._rec = torch.from_numpy(REC_THRS.astype(np.float64)).to(dev)
        self._area = torch.from_numpy(np.array(AREA_RNG, dtype=np.float64).reshape(-1)).to(dev)
        self._maxdets = torch.tensor(MAX_DETS, dtype=torch.int32).to(dev)
        self._h_maxdets = (ctypes.c_int * len(MAX_DETS))(*MAX_DETS)
        self.result = None
        self.iou_row_gts = gt.max_pair_gts      # IoU row kept in LDS; pairs with more GTs recompute (same bits)
        self.reset()

    def reset(self):
        self._chunks = []
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.result = None

    @property
    def num_records(self):
        return sum(int(c[1].numel()) for c in self._chunks)

    def add(self, dets, count, im_ids):
        """One batch of `forward_padded` / `Ticket.padded()` results (dets [N, keep_k, 6] float32, count [N] int32, on the
        device) for the images `im_ids` (host sequence of N image ids), enqueued on the current stream without a host
        sync.  The rows are turned into records (the reference writer's arithmetic) in a buffer of the evaluator's, so the
        next forward may overwrite `dets`."""
        if not (dets.is_cuda and count.is_cuda):
            raise _lib.PPYoloHipError('BboxEvaluator.add takes the device tensors of forward_padded (no CPU path)')
        if dets.dim() != 3 or dets.shape[2] != 6 or dets.dtype != torch.float32:
            raise ValueError('dets must be [N, keep_k, 6] float32')
        N, keep_k = int(dets.shape[0]), int(dets.shape[1])
        if len(im_ids) != N or count.numel() != N:
            raise ValueError('one image id and one count per image')
        idx = []
        for v in im_ids:
            i = self.gt.img_index.get(int(v))
            if i is None:
                raise ValueError('Results do not correspond to current coco set: image_id %r' % (v,))
            idx.append(i)
        img = torch.tensor(idx, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        dets = dets.contiguous()
        count = count.to(torch.int32).contiguous()
        rec = torch.empty((N * keep_k, 6), dtype=torch.float64, device=self.device)
        pair = torch.empty(N * keep_k, dtype=torch.int32, device=self.device)
        check(lib().ppy_cocoeval_records_f32(dets.data_ptr(), N, keep_k, count.data_ptr(), img.data_ptr(), self._cls2k.data_ptr(),
                                             self._ncls, self.gt.num_cats, rec.data_ptr(), pair.data_ptr(), self._bad.data_ptr(),
                                             _stream()), 'ppy_cocoeval_records_f32')
        self._chunks.append((rec, pair, img))
        self.result = None

    def records(self):
        """The device records so far as host arrays (rec [n, 6], pair [n]; pair -1 = not a record)."""
        if not self._chunks:
            return np.zeros((0, 6)), np.zeros(0, dtype=np.int32)
        return (torch.cat([c[0] for c in self._chunks]).cpu().numpy(), torch.cat([c[1] for c in self._chunks]).cpu().numpy())

    def add_records(self, records):
        """Result records as the reference writes them ({'image_id', 'category_id', 'bbox': [x, y, w, h], 'score'}),
        parsed on the host and uploaded.  Records of categories outside the GT are dropped."""
        rec, pair = records_to_arrays(self.gt, records)
        if len(pair) == 0:
            return
        self._chunks.append((torch.from_numpy(rec).to(self.device), torch.from_numpy(pair).to(self.device), None))
        self.result = None

    def run(self):
        """Enqueue evaluate + accumulate on the current stream -> device (precision, recall, scores); no host sync."""
        gt = self.gt
        dev = self.device
        if self._chunks:
            rec = torch.cat([c[0] for c in self._chunks]) if len(self._chunks) > 1 else self._chunks[0][0]
            pair = torch.cat([c[1] for c in self._chunks]) if len(self._chunks) > 1 else self._chunks[0][1]
        else:
            rec = torch.zeros((0, 6), dtype=torch.float64, device=dev)
            pair = torch.zeros(0, dtype=torch.int32, device=dev)
        n = int(pair.numel())
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), gt.num_cats, len(AREA_RNG), len(MAX_DETS)
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        wsb = int(lib().ppy_cocoeval_workspace_bytes(n, gt.num_images, K, gt.num_gts, T, A, M))
        if wsb == 0:
            raise _lib.PPYoloHipError('ppy_cocoeval_workspace_bytes rejected the sizes')
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        nz = gt.num_gts > 0
        check(lib().ppy_cocoeval_bbox(rec.data_ptr() if n else None, pair.data_ptr() if n else None, n, gt.num_images, K,
                                      gt.d_off.data_ptr(), gt.d_box.data_ptr() if nz else None,
                                      gt.d_area.data_ptr() if nz else None, gt.d_crowd.data_ptr() if nz else None,
                                      gt.d_idnz.data_ptr() if nz else None, gt.d_cat_off.data_ptr(), gt.num_gts, int(self.iou_row_gts),
                                      self._iou.data_ptr(), T, self._rec.data_ptr(), R, self._area.data_ptr(), A,
                                      self._maxdets.data_ptr(), self._h_maxdets, M, precision.data_ptr(), recall.data_ptr(),
                                      scores.data_ptr(), ws.data_ptr(), wsb, _stream()), 'ppy_cocoeval_bbox')
        return precision, recall, scores

    def evaluate(self):
        """evaluate() + accumulate() -> dict(precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M] float64 numpy,
        stats [12]) -- COCOeval.eval plus COCOeval.stats."""
        precision, recall, scores = self.run()
        if int(self._bad.item()):
            raise ValueError('NaN in a detection row given to BboxEvaluator.add')
        p, r, s = precision.cpu().numpy(), recall.cpu().numpy(), scores.cpu().numpy()
        self.result = dict(precision=p, recall=r, scores=s, stats=summarize_stats(p, r))
        return self.result

    @property
    def stats(self):
        return None if self.result is None else self.result['stats']

    def summarize(self):
        """Print pycocotools' 12 summary lines; returns the stats."""
        if self.result is None:
            self.evaluate()
        lines = []
        stats = summarize_stats(self.result['precision'], self.result['recall'], lines)
        print('\n'.join(lines))
        return stats

