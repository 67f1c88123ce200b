"""Matrix-NMS against multiclass_nms on the flagship workload (R50vd-608, batch 8, synthetic weights, seeded inputs, as bench.py
builds them), in ONE process with the legs alternating:

  1. the NMS launches alone, on the same decoded buffers (boxes + candidate lists of the step): the normal regime (the step's
     own head outputs) and the all-pass regime (head logits ~ N(0, 0.1): every (box, class) pair is a candidate);
  2. the one-batch-at-a-time forward (one executor, one hipGraph replay per step) with each nms_type.

Every figure is the median of `--rounds` windows of at least `--seconds` (host clock around launches that end in a device
synchronise), the two legs of a comparison taking turns window by window; the spread (min .. max) is printed beside it.

    python tools/nms_bench.py [--out profiles/nms_bench.txt] [--seconds 1.0] [--rounds 5]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
import bench  # noqa: E402
from config import multiclass_nms_defaults  # noqa: E402
from ppyolo_hip import ops as K, synth  # noqa: E402


def window(fn, seconds):
    """-> seconds per call of fn over a window of at least `seconds` (fn enqueues; the window ends in a synchronise)."""
    n = 4
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n
        n = max(n + 1, int(n * min(8.0, 1.15 * seconds / max(dt, 1e-6))))


def alternate(legs, seconds, rounds):
    """legs: {name: fn} -> {name: (median, min, max)} seconds per call, the legs taking turns window by window."""
    for fn in legs.values():      # warm-up: code objects, graphs
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(window(fn, seconds))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nms_bench.txt'))
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nms_bench needs the MI355X: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    x = synth.synth_images(8, 608).to(dev)
    ims = synth.synth_im_size(8).to(dev)
    models = {}
    for name in ('matrix_nms', 'multiclass_nms'):
        model, sd, cfg = bench.build_model('PPYOLO_2x_Config', dev)
        if name == 'multiclass_nms':
            model.head.nms_cfg = multiclass_nms_defaults()      # (read when the plan is built, at the first forward)
        ex = model._plans.executor(x)
        ex.set_inputs(x, ims)
        ex.run()
        ex.run()
        torch.cuda.synchronize()
        assert ex.plan.decode['nms_type'] == name
        models[name] = (model, ex)
    say('R50vd-608, batch 8, synthetic weights (seed 0), seeded inputs; windows >= %.1f s, %d rounds, legs alternating' % (a.seconds, a.rounds))
    say('nms_cfg  matrix_nms     : %r' % (models['matrix_nms'][1].plan.decode['nms'],))
    say('nms_cfg  multiclass_nms : %r' % (models['multiclass_nms'][1].plan.decode['nms'],))
    say()

    # ---- 1. the NMS launches alone, both on the Matrix-NMS executor's decoded buffers ----
    ex = models['matrix_nms'][1]
    d = ex.plan.decode
    n, mc = d['nms'], models['multiclass_nms'][1].plan.decode['nms']
    heads = [ex.view(h) for h in ex.plan.head_outs]
    C = d['num_classes']
    mc_ws = K.multiclass_nms_workspace(8, C, mc['nms_top_k'], ex.cand_key.shape[1], dev)
    mc_out = (torch.zeros((8, mc['keep_top_k'], 6), device=dev), torch.zeros((8,), dtype=torch.int32, device=dev),
              torch.zeros((8, mc['keep_top_k']), dtype=torch.int32, device=dev))

    def decode():
        ex.cand_count.zero_()
        K.yolo_decode_levels(heads, [lvl['anchors'] for lvl in d['levels']], [lvl['downsample'] for lvl in d['levels']], C,
                             d['scale_x_y'], d['iou_aware'], d['iou_aware_factor'], d['clip_bbox'], ex.im_size, ex.boxes,
                             n['score_threshold'], ex.cand_key, ex.cand_idx, ex.cand_count)

    def matrix():
        K.matrix_nms(ex.boxes, C, ex.cand_key, ex.cand_idx, ex.cand_count, n['post_threshold'], n['nms_top_k'], n['keep_top_k'],
                     n['use_gaussian'], n['gaussian_sigma'], ex.out_dets, ex.out_count, ex.out_keep, ex.nms_ws)

    def multiclass():
        K.multiclass_nms(ex.boxes, C, ex.cand_key, ex.cand_idx, ex.cand_count, mc['nms_top_k'], mc['keep_top_k'], mc['nms_threshold'],
                         mc['normalized'], mc['nms_eta'], mc['background_label'], mc_out[0], mc_out[1], mc_out[2], mc_ws)

    def nms_regime(label):
        decode()
        torch.cuda.synchronize()
        cands = ex.cand_count.cpu().tolist()
        r = alternate(dict(matrix_nms=matrix, multiclass_nms=multiclass), a.seconds, a.rounds)
        say('NMS launches alone, %s: candidates per image %d .. %d (mean %d)' % (label, min(cands), max(cands), sum(cands) // len(cands)))
        for k in ('matrix_nms', 'multiclass_nms'):
            cnt = (ex.out_count if k == 'matrix_nms' else mc_out[1]).cpu().tolist()
            say('  %-15s %10.1f us per step   (%.1f .. %.1f)   detections per image %d .. %d' % (
                k, r[k][0] * 1e6, r[k][1] * 1e6, r[k][2] * 1e6, min(cnt), max(cnt)))
        say('  multiclass_nms - matrix_nms = %+.1f us per step' % ((r['multiclass_nms'][0] - r['matrix_nms'][0]) * 1e6))
        say()

    nms_regime('normal regime (the step\'s own head outputs, score_threshold %.2f)' % n['score_threshold'])
    saved = [h.t.clone() for h in heads]
    g = torch.Generator(device=dev).manual_seed(7)
    for h in heads:
        h.t.copy_(torch.randn(h.t.shape, generator=g, device=dev) * 0.1)      # logits ~ 0: score ~ 0.25 everywhere
    try:
        nms_regime('all-pass regime (head logits ~ N(0, 0.1))')
    finally:
        for h, sv in zip(heads, saved):
            h.t.copy_(sv)
        decode()
        matrix()
        torch.cuda.synchronize()

    # ---- 2. the whole forward, one batch at a time ----
    r = alternate({k: v[1].run for k, v in models.items()}, a.seconds, a.rounds)
    say('forward, one batch at a time (hipGraph replay, batch 8), normal regime')
    for k in ('matrix_nms', 'multiclass_nms'):
        say('  %-15s %8.1f images/s   %7.3f ms per step   (%.3f .. %.3f ms)' % (k, 8 / r[k][0], r[k][0] * 1e3, r[k][1] * 1e3, r[k][2] * 1e3))
    ratio = r['matrix_nms'][0] / r['multiclass_nms'][0]
    say('  multiclass_nms / matrix_nms rate = %.4f (%+.2f %%); condition: no more than 3 %% below -> %s' % (
        ratio, (ratio - 1) * 100, 'MET' if ratio >= 0.97 else 'MISSED'))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
