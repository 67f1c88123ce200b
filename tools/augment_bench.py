"""Training-batch builder timings (ppyolo_hip/augment.py, csrc/augment.hip).

    python tools/augment_bench.py [--bs 8] [--iters 20] [--sources host|device|files|all] [--rounds 1]

Reports: host plan time per batch (the reference's transforms, draw for draw, no pixel work); device time of the render
and target kernels (HIP events) at bs 8 for S = 320 and 608 and every interpolation, on 640 x 480 sources through the
full chain (mixup partners, colour ops, expand, crop, flip as drawn); the builder feeding TrainStep.step (steps/s, builder
on a producer thread one batch ahead).

--sources names where the builder's pixels come from, one leg each under "sources" of the JSON line: host (numpy images,
packed into the blob and uploaded per batch), device (the same images uploaded once, read in place), files (the COCO-sized
JPEG fixtures as bytes, decoded on the device inside every call: from_files).  Per leg: blob_bytes, call_ms (host wall time
of one builder call, plan included), call_sync_ms (until the batch is there), train_steps_per_s (median of --rounds rounds,
the legs alternating, every round listed); for host also call_split_ms: the call's stages timed in place, plan (with the
target records) / pack_batch / pin_memory / upload (enqueue) / launch (output buffers + the two launches)."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd')]

from config import PPYOLO_2x_Config  # noqa: E402
from ppyolo_hip import augment as A, ops, targets as T  # noqa: E402
from ppyolo_hip.jpeg import JpegDecoder  # noqa: E402


def samples(rng, n, hw=(480, 640)):
    out = []
    for k in range(n):
        def one():
            G = int(rng.randint(1, 20))
            h, w = hw
            x1, y1 = rng.uniform(0, w - 60, G), rng.uniform(0, h - 60, G)
            box = np.stack([x1, y1, x1 + rng.uniform(20, 60, G), y1 + rng.uniform(20, 60, G)], 1).astype(np.float32)
            return dict(image=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), h=h, w=w, gt_bbox=box,
                        gt_class=rng.randint(0, 80, (G, 1)).astype(np.int32), gt_score=np.ones((G, 1), np.float32),
                        is_crowd=np.zeros((G, 1), np.int32))
        s = one()
        s['mixup'] = one()
        out.append(s)
    return out


def file_records(rng, n):
    """n records with mixup partners whose images are the COCO-sized JPEG fixtures (tests/golden/g20_jpeg.npz, the files
    tools/jpeg_bench.py replicates), as bytes; boxes as in samples()."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    big = [(g['jpg_' + str(nm)].tobytes(), tuple(int(v) for v in g['shape_' + str(nm)][:2])) for nm in g['names']
           if str(nm).startswith('coco_')]
    out = []
    for k in range(n):
        def one(j):
            data, hw = big[j % len(big)]
            r = samples(rng, 1, hw)[0]
            r.pop('mixup')
            r['image'] = data
            return r
        s = one(k)
        s['mixup'] = one(k + 1)
        out.append(s)
    return out


def ev_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--train-steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--sources', choices=['host', 'device', 'files', 'all'], default='host')
    a = ap.parse_args()
    cfg = PPYOLO_2x_Config()
    b = A.TrainBatchBuilder(cfg)
    rng = np.random.RandomState(0)
    batch = samples(rng, a.bs)
    res = dict(bs=a.bs)
    t0 = time.perf_counter()
    for i in range(a.iters):
        b.plan(batch, 608, np.random.RandomState(i))
    res['plan_ms'] = (time.perf_counter() - t0) * 1e3 / a.iters
    lut = torch.from_numpy(b.lut_np).cuda()
    res['render_ms'], res['targets_ms'] = {}, {}
    for S in (320, 608):
        for interp in A.INTERPS:
            b.random_inter = False
            recipes, bb, cl, sc = b.plan(batch, S, np.random.RandomState(1))
            for r in recipes:           # force the interpolation, keep the drawn chain
                r['interp'] = interp
                r['resize'] = A.resize_plan(r['crop'][2], r['crop'][3], r['fx'], r['fy'], interp, r['canvas_dtype'])
            o, v = T.gt2yolo_records(bb, cl, sc, b.anchors, b.anchor_masks, b.downsample_ratios, 80, S)
            blob, lay = A.pack_batch(recipes, True, o, v, bb, cl, sc)
            dev = torch.from_numpy(blob).cuda()
            out = torch.empty((a.bs, 3, S, S), device='cuda')
            res['render_ms']['%d_%d' % (S, interp)] = ev_time(
                lambda: ops.augment_render(dev, a.bs, S, lut, b.mean, b.std, out), a.iters)
            if interp == A.INTERPS[0]:
                total = sum(a.bs * len(m) * 86 * (S // d) ** 2 for m, d in zip(b.anchor_masks, b.downsample_ratios))
                flat = torch.empty(total, device='cuda')
                res['targets_ms'][str(S)] = ev_time(lambda: ops.augment_targets(flat, dev, lay['toff'], lay['tval'], len(o)), a.iters)
    b.random_inter = True
    legs = ['host', 'device', 'files'] if a.sources == 'all' else [a.sources]
    feeds = {}
    if 'host' in legs:
        feeds['host'] = lambda i: b(batch, 608, np.random.RandomState(100 + i))
    if 'device' in legs:            # the same images, uploaded once before anything is timed
        up = lambda r: dict(r, image=torch.from_numpy(r['image']).cuda())
        dev_batch = [dict(up(r), mixup=up(r['mixup'])) for r in batch]
        feeds['device'] = lambda i: b(dev_batch, 608, np.random.RandomState(100 + i))
    if 'files' in legs:             # JPEG bytes in, decoded on the device inside every call
        recs = file_records(np.random.RandomState(0), a.bs)
        dec = JpegDecoder()
        feeds['files'] = lambda i: b.from_files(recs, 608, np.random.RandomState(100 + i), decoder=dec)
    res['sources'] = {}
    for leg in legs:
        r = res['sources'][leg] = {}
        feeds[leg](0)
        torch.cuda.synchronize()
        r['blob_bytes'] = int(b._keep[1].numel())
        t0 = time.perf_counter()
        for i in range(a.iters):
            feeds[leg](i)
        r['call_ms'] = (time.perf_counter() - t0) * 1e3 / a.iters           # host wall time of a call, plan included
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.iters):
            feeds[leg](i)
            torch.cuda.synchronize()
        r['call_sync_ms'] = (time.perf_counter() - t0) * 1e3 / a.iters      # ... and until the batch is there
    if 'host' in legs:              # where the host leg's call goes: the stages of __call__, back to back as in the loop above
        r, t = res['sources']['host'], dict(plan=0.0, pack=0.0, pin=0.0, upload=0.0, launch=0.0)
        keep = None
        for i in range(a.iters):
            t0 = time.perf_counter()
            recipes, bb, cl, sc = b.plan(batch, 608, np.random.RandomState(100 + i))
            o, v = T.gt2yolo_records(bb, cl, sc, b.anchors, b.anchor_masks, b.downsample_ratios, b.num_classes, 608, b.iou_thresh)
            t1 = time.perf_counter()
            blob, lay = A.pack_batch(recipes, b.to_rgb, o, v, bb, cl, sc)
            t2 = time.perf_counter()
            pinned = torch.from_numpy(blob).pin_memory()
            t3 = time.perf_counter()
            dev = pinned.to('cuda', non_blocking=True)
            t4 = time.perf_counter()
            out = torch.empty((a.bs, 3, 608, 608), device='cuda')
            flat = torch.empty(sum(a.bs * len(m) * (6 + b.num_classes) * (608 // d) ** 2
                                   for m, d in zip(b.anchor_masks, b.downsample_ratios)), device='cuda')
            ops.augment_render(dev, a.bs, 608, lut, b.mean, b.std, out, b.is_scale)
            ops.augment_targets(flat, dev, lay['toff'], lay['tval'], len(o))
            keep = (pinned, dev, out, flat)         # as the builder holds its last batch
            t5 = time.perf_counter()
            for k, x in zip(('plan', 'pack', 'pin', 'upload', 'launch'), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                t[k] += x
        torch.cuda.synchronize()
        r['call_split_ms'] = {k: x * 1e3 / a.iters for k, x in t.items()}
    # the builder feeding the training step, one batch ahead on a producer thread
    try:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from conftest import build_model
        from ppyolo_hip.train import TrainStep
        model, _ = build_model(cfg, 0, 'cuda')
        ts = TrainStep(model, cfg)
        side = torch.cuda.Stream()

        def train_leg(feed):
            q = []
            ready = threading.Semaphore(0)

            def produce(i):
                with torch.cuda.stream(side):
                    d = feed(i)
                    e = torch.cuda.Event()
                    e.record(side)
                q.append((d, e))
                ready.release()
            th = threading.Thread(target=produce, args=(0,))
            th.start()
            for it in range(a.train_steps + 2):
                if it == 2:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                ready.acquire()
                th.join()
                d, e = q.pop(0)
                th = threading.Thread(target=produce, args=(it + 1,))
                th.start()
                torch.cuda.current_stream().wait_event(e)
                ts.step(d['images'], d['gt_bbox'], [d['target0'], d['target1'], d['target2']], 1e-4)
            torch.cuda.synchronize()
            rate = a.train_steps / (time.perf_counter() - t0)
            th.join()
            return rate

        for rnd in range(a.rounds):             # the legs alternate, every round is reported: the spread is in the output
            for leg in legs:
                res['sources'][leg].setdefault('train_steps_per_s_rounds', []).append(train_leg(feeds[leg]))
        for leg in legs:
            res['sources'][leg]['train_steps_per_s'] = float(np.median(res['sources'][leg]['train_steps_per_s_rounds']))
        if 'host' in legs:
            res['train_steps_per_s'] = res['sources']['host']['train_steps_per_s']
    except Exception as ex:          # report, do not hide
        res['train_error'] = repr(ex)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
