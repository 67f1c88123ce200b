"""Timings of test-time augmentation (ppyolo_hip/tta.py; csrc/fuse_views.hip: ppy_fuse_views_f32, one launch, one workgroup per
image) on a batch of 8 images 640 x 480 at R50vd with the synthetic weights: input sides 512, 608 and 704, each plain and mirrored
-> 48 views, six forward chunks of 8, none padded.  ONE process, the legs alternating:

  (a) fuse, own rows       the fuse launch alone on the rows this very run's 48 views produced, replayed from a captured graph;
  (b) fuse, clustered      tests/fuse_views_ref.spread_case(0, 41): 700 rows of the NMS tests' clustered recipe dealt to 41 views,
                           mirrors on half of them, about 550 admitted, one image;
  (c) fuse, worst case     8192 admitted rows of ONE image in ONE class (tests/fuse_views_ref.uniform_case with the class set to
                           0): one class segment, so one wave walks every row, each against every cluster so far;
  (d) merge_views          ppy_merge_views_f32 ('iou', the same threshold) on the rows of (a) and of (b): the suppression the
                           fusion is not, as the yardstick of a view merge that has no serial chain;
  (e) forward chunk        pre-processing of 8 images + forward_padded at 608 (and at 512, the smallest side of the call), and the
                           whole TtaDetector call;
  (f) what the parent commit would have to do instead of (a): copy dets [V, K, 6] and count to the host (the copy and its
      synchronisation alone), then loop in numpy (the restatement of tests/fuse_views_ref.py on those rows, and on (b)'s).

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.  Aim 1: (a) and (b) each < one forward chunk (e), so that a fusion can hide behind the next
batch's first chunk.  Aim 2 (reported, no condition): (a) / (d) and (b) / (d).  (c) is reported without a condition.

    python tools/tta_bench.py [--out profiles/tta_bench.txt] [--seconds 1.0] [--rounds 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fuse_views_ref as R  # noqa: E402
from jpeg_encode_bench import alternate, graph_of  # noqa: E402
from tile_bench import merge_call  # noqa: E402
from ppyolo_hip import ops  # noqa: E402
from ppyolo_hip.tiles import preprocess_views  # noqa: E402
from ppyolo_hip.tta import TtaDetector  # noqa: E402

H, W, BS, SCALES = 480, 640, 8, (512, 608, 704)


def batch():
    """Eight 640 x 480 device images: the 640-wide COCO fixture, rolled sideways by a different amount each."""
    from ppyolo_hip.jpeg import JpegDecoder
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    files = [g['jpg_' + str(n)].tobytes() for n in g['names'] if str(n).startswith('coco_')]
    im = max(JpegDecoder().decode(files), key=lambda t: t.shape[1])
    im = im.repeat(-(-H // im.shape[0]), -(-W // im.shape[1]), 1)[:H, :W]
    return [torch.roll(im, 67 * i, dims=1).contiguous() for i in range(BS)]


def fuse_call(dets, count, table, weight, n, kw):
    """One ppy_fuse_views_f32 call on fixed device rows, as a closure a graph can capture."""
    d_dets = dets if isinstance(dets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dets)).cuda()
    d_count = count if isinstance(count, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(count)).cuda()
    tab = ops.fuse_views_table(table)
    w = np.ascontiguousarray(weight, dtype=np.float32)
    d_tab, d_w = torch.from_numpy(tab).cuda(), torch.from_numpy(w).cuda()
    V, K = d_dets.shape[0], d_dets.shape[1]
    ws = ops.fuse_views_workspace(n, V, K, 'cuda')
    k = kw['keep_top_k']
    out = (torch.empty((n, k, 6), dtype=torch.float32, device='cuda'), torch.empty((n,), dtype=torch.int32, device='cuda'),
           torch.empty((n, k, 2), dtype=torch.int32, device='cuda'), torch.empty((n, k), dtype=torch.int32, device='cuda'))
    run = lambda: ops.fuse_views(d_dets, d_count, tab, d_tab, w, d_w, n, kw['thresh'], kw['score_thresh'], k, *out, ws=ws)      # noqa: E731
    run.out, run.keep = out, (d_dets, d_count, d_tab, d_w, ws)
    return run


def total(stats, key, fn=sum):
    return fn(s[key] for s in stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tta_bench.txt'))
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tta_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    from config import PPYOLO_2x_Config
    from conftest import build_model
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg, 0, 'cuda')
    images = batch()
    tta = TtaDetector(model, cfg, scales=SCALES, hflip=True, batch=BS)
    got = tta(images)
    torch.cuda.synchronize()
    _, blob, all_dets, all_count, _ = tta._keep
    V, K = all_dets.shape[0], all_dets.shape[1]
    table = [(i, 0, 0, W if f else 0) for i, S, f in tta.views]
    weight = np.ones((V,), dtype=np.float32)
    kw = dict(thresh=tta.thresh, score_thresh=tta.score_thresh, keep_top_k=tta.keep_top_k)
    h_dets, h_count = all_dets.cpu().numpy(), all_count.cpu().numpy()
    st = []
    want = R.fuse_views(h_dets, h_count, np.array(table), weight, BS, stats=st, **kw)
    say('%d images %d x %d, input sides %s, plain and mirrored: %d views in %d chunks of %d; R50vd, synthetic weights; %s; windows '
        '>= %.1f s, %d rounds, legs alternating' % (BS, W, H, SCALES, V, V // BS, BS, torch.cuda.get_device_name(0), a.seconds, a.rounds))
    say("the run's own rows: K = %d, %d rows reported by the views, %d admitted at score_thresh %g, %d clusters (IoU > %g), the largest "
        'of %d rows, %d singletons' % (K, int(h_count.sum()), total(st, 'admitted'), kw['score_thresh'], total(st, 'clusters'),
                                       kw['thresh'], total(st, 'max_members', max), total(st, 'singletons')))
    for g, w in zip(got, want):
        assert g.cpu().numpy().tobytes() == w.tobytes(), 'TtaDetector differs from the restatement on its own rows'

    legs, names, keep = {}, {}, []

    def add(key, name, fn):
        legs[key], names[key] = fn, name

    clus = R.spread_case(0, 41)
    stc = []
    R.run(clus, stats=stc)
    ckw = dict(clus['kw'], keep_top_k=kw['keep_top_k'])
    worst = R.one_class_case(*R.BOUNDARIES[-1], keep_top_k=kw['keep_top_k'])
    stw = []
    R.run(worst, stats=stw)
    miou = dict(metric='iou', class_agnostic=False)
    calls = [('own', "(a) fuse, the run's own rows (%d admitted, %d clusters)" % (total(st, 'admitted'), total(st, 'clusters')),
              fuse_call(all_dets.clone(), all_count.clone(), table, weight, BS, kw)),
             ('clus', '(b) fuse, clustered recipe in 41 views (%d admitted, %d clusters)' % (stc[0]['admitted'], stc[0]['clusters']),
              fuse_call(clus['dets'], clus['count'], clus['views'], clus['weight'], 1, ckw)),
             ('worst', '(c) fuse, 8192 admitted rows of one image in one class (%d clusters)' % stw[0]['clusters'],
              fuse_call(worst['dets'], worst['count'], worst['views'], worst['weight'], 1, worst['kw'])),
             ('mown', "(d) merge_views ('iou') on the rows of (a)",
              merge_call(all_dets.clone(), all_count.clone(), [t[:3] for t in table], BS, dict(kw, **miou))),
             ('mclus', "(d) merge_views ('iou') on the rows of (b)",
              merge_call(clus['dets'], clus['count'], clus['views'][:, :3], 1, dict(ckw, **miou)))]
    for key, name, run in calls:
        keep.append(run)
        add(key, name, graph_of(run))

    sizes8 = torch.tensor([[H, W]] * BS, dtype=torch.float32).cuda()

    def forward_chunk(pre):
        def run():
            x, im_size = preprocess_views(pre, images, sizes8)
            return model.forward_padded(x, im_size)
        return run
    add('chunk608', '(e) one forward chunk at 608: 8 images pre-processed + forward_padded', forward_chunk(tta.pre[SCALES.index(608)]))
    add('chunk512', '(e) one forward chunk at 512', forward_chunk(tta.pre[SCALES.index(512)]))
    add('tta', '(e) the whole TtaDetector call (%d chunks + flips + fuse)' % (V // BS), lambda: tta(images))

    def read_back():
        return all_dets.cpu(), all_count.cpu()
    add('copy', '(f) copy of dets [%d, %d, 6] and count to the host, with its synchronisation' % (V, K), read_back)
    add('numpy', "(f) numpy restatement on the run's own rows",
        lambda: R.fuse_views(h_dets, h_count, np.array(table), weight, BS, **kw))
    add('numpyc', '(f) numpy restatement on the clustered recipe', lambda: R.run(clus, keep_top_k=kw['keep_top_k']))

    r = alternate(legs, a.seconds, a.rounds)
    say()
    for k in legs:
        say('%-86s %9.3f ms   (%.3f .. %.3f)' % (names[k], r[k][0] * 1e3, r[k][1] * 1e3, r[k][2] * 1e3))
    say()
    for key, what in (('own', "(a) the run's own rows"), ('clus', '(b) the clustered recipe')):
        for ck in ('chunk608', 'chunk512'):
            say('aim 1: fuse of %s %.3f ms < one forward chunk (%s) %.3f ms -> %s (%.1f %% of a chunk)' % (
                what, r[key][0] * 1e3, ck[5:], r[ck][0] * 1e3, 'MET' if r[key][0] < r[ck][0] else 'MISSED', 100 * r[key][0] / r[ck][0]))
    say('aim 2 (no condition): fuse / merge_views = %.2fx on the rows of (a), %.2fx on the rows of (b)' % (
        r['own'][0] / r['mown'][0], r['clus'][0] / r['mclus'][0]))
    say('(c), no condition: %.3f ms = %.2f forward chunks at 608' % (r['worst'][0] * 1e3, r['worst'][0] / r['chunk608'][0]))
    say("finding: the fusion is %.2f %% of the whole TTA call; the parent's path (copy + numpy, own rows) would take %.3f ms" % (
        100 * r['own'][0] / r['tta'][0], (r['copy'][0] + r['numpy'][0]) * 1e3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
