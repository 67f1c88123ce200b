"""Timings of tiled inference (ppyolo_hip/tiles.py; csrc/merge_views.hip: ppy_merge_views_f32, one launch, one workgroup per
image) on one 3840 x 2160 image at R50vd-608 with the synthetic weights: tile 608, overlap 0.2, the whole image first -> 41 views,
six forward chunks of 8 (the last one filled with 7 padding views).  ONE process, the legs alternating:

  (a) merge, own rows      the merge launch alone on the rows this very run's 41 views produced, replayed from a captured graph;
  (b) merge, worst case    8192 admitted rows in one image (64 views x 128 rows, tests/tile_merge_ref.uniform_case: boxes placed
                           uniformly, a box meets a handful of others): the bitonic network over the full stage, and a scan that
                           runs until keep_top_k selections are found -- with the configuration's keep_top_k = 100 and with the
                           largest, 1024;
  (c) merge, clustered     tests/tile_merge_ref.spread_case(0, 41, 100): 700 rows of the NMS tests' clustered recipe dealt to 41
                           views, about 550 admitted;
  (d) forward chunk        pre-processing of 8 views in place + forward_padded, and the whole TiledDetector call;
  (e) what the parent commit would have to do instead of (a): copy dets [V, K, 6] and count to the host (the copy and its
      synchronisation alone), then loop in numpy (the restatement of tests/tile_merge_ref.py on those rows, and on (c)'s).

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.  The aims: (b) < one forward chunk (d), so that a merge can hide behind the next image's
first chunk; (a) <= the read-back alone of (e).

    python tools/tile_bench.py [--out profiles/tile_bench.txt] [--seconds 1.0] [--rounds 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tile_merge_ref as R  # noqa: E402
from jpeg_encode_bench import alternate, graph_of  # noqa: E402
from ppyolo_hip import ops  # noqa: E402
from ppyolo_hip.tiles import TiledDetector, preprocess_views  # noqa: E402

H, W, S, BS = 2160, 3840, 608, 8


def frame():
    """A 3840 x 2160 device image: the 640-wide COCO fixture repeated (synthetic weights see structure, not noise)."""
    from ppyolo_hip.jpeg import JpegDecoder
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    files = [g['jpg_' + str(n)].tobytes() for n in g['names'] if str(n).startswith('coco_')]
    im = max(JpegDecoder().decode(files), key=lambda t: t.shape[1])
    reps = (-(-H // im.shape[0]), -(-W // im.shape[1]), 1)
    return im.repeat(*reps)[:H, :W].contiguous()


def merge_call(dets, count, table, n, kw):
    """One ppy_merge_views_f32 call on fixed device rows, as a closure a graph can capture."""
    d_dets = dets if isinstance(dets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dets)).cuda()
    d_count = count if isinstance(count, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(count)).cuda()
    tab = ops.merge_views_table(table)
    d_tab = torch.from_numpy(tab).cuda()
    V, K = d_dets.shape[0], d_dets.shape[1]
    ws = ops.merge_views_workspace(n, V, K, 'cuda')
    k = kw['keep_top_k']
    out = (torch.empty((n, k, 6), dtype=torch.float32, device='cuda'), torch.empty((n,), dtype=torch.int32, device='cuda'),
           torch.empty((n, k, 2), dtype=torch.int32, device='cuda'))
    run = lambda: ops.merge_views(d_dets, d_count, tab, d_tab, n, kw['metric'], kw['thresh'], kw['score_thresh'],      # noqa: E731
                                  kw['class_agnostic'], k, *out, ws=ws)
    run.out, run.keep = out, (d_dets, d_count, d_tab, ws)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tile_bench.txt'))
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tile_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    from config import PPYOLO_2x_Config
    from conftest import build_model
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg, 0, 'cuda')
    img = frame()
    tiled = TiledDetector(model, cfg, S, batch=BS)
    dets, count, src = tiled([img])
    torch.cuda.synchronize()
    views = tiled.views
    _, _, all_dets, all_count, _ = tiled._keep
    V, K = all_dets.shape[0], all_dets.shape[1]
    table = [(v[0], v[1], v[2]) for v in views] + [(-1, 0, 0)] * (V - len(views))
    kw = dict(metric=tiled.metric, thresh=tiled.thresh, score_thresh=tiled.score_thresh, class_agnostic=False, keep_top_k=tiled.keep_top_k)
    h_dets, h_count = all_dets.cpu().numpy(), all_count.cpu().numpy()
    st = []
    want = R.merge_views(h_dets, h_count, np.array(table), 1, stats=st, **kw)
    say('one %d x %d image, tile %d, overlap %.1f, full view: %d views in %d chunks of %d; R50vd-%d, synthetic weights; %s; windows '
        '>= %.1f s, %d rounds, legs alternating' % (W, H, S, tiled.overlap, len(views), V // BS, BS, S, torch.cuda.get_device_name(0),
                                                    a.seconds, a.rounds))
    say("the run's own rows: K = %d, %d rows reported by the views, %d admitted at score_thresh %g, %d selected, %d suppressed ('%s' at %g)"
        % (K, int(h_count[:len(views)].sum()), st[0]['admitted'], kw['score_thresh'], st[0]['selected'], st[0]['suppressed'], kw['metric'],
           kw['thresh']))
    for g, w in zip((dets, count, src), want):
        assert g.cpu().numpy().tobytes() == w.tobytes(), 'TiledDetector differs from the restatement on its own rows'

    legs, names, keep = {}, {}, []

    def add(key, name, fn):
        legs[key], names[key] = fn, name

    own = merge_call(all_dets.clone(), all_count.clone(), table, 1, kw)
    worst = R.uniform_case(*R.BOUNDARIES[-1])
    clus = R.spread_case(0, 41, 100)
    calls = [('own', '(a) merge, the run\'s own rows (%d admitted)' % st[0]['admitted'], own)]
    for keep_k in (kw['keep_top_k'], 1024):
        p = dict(worst['kw'], keep_top_k=keep_k)
        calls.append(('worst%d' % keep_k, '(b) merge, 8192 admitted rows uniform, keep_top_k %d' % keep_k,
                      merge_call(worst['dets'], worst['count'], worst['views'], 1, p)))
    stc = []
    R.run(clus, stats=stc)
    calls.append(('clus', '(c) merge, clustered recipe in 41 views (%d admitted, %d selected)' % (stc[0]['admitted'], stc[0]['selected']),
                  merge_call(clus['dets'], clus['count'], clus['views'], 1, dict(clus['kw'], keep_top_k=kw['keep_top_k']))))
    for key, name, run in calls:
        keep.append(run)
        add(key, name, graph_of(run))

    chunk = tiled.chunks(views)[1]          # eight tiles of the first tile row
    tiles8 = tiled.view_tensors([img], chunk)

    sizes8 = torch.tensor([[t.shape[0], t.shape[1]] for t in tiles8], dtype=torch.float32).cuda()

    def forward_chunk():
        x, im_size = preprocess_views(tiled.pre, tiles8, sizes8)
        return model.forward_padded(x, im_size)
    add('chunk', '(d) one forward chunk: 8 views pre-processed in place + forward_padded', forward_chunk)
    add('tiled', '(d) the whole TiledDetector call (%d chunks + merge)' % (V // BS), lambda: tiled([img]))

    def read_back():
        return all_dets.cpu(), all_count.cpu()
    add('copy', '(e) copy of dets [%d, %d, 6] and count to the host, with its synchronisation' % (V, K), read_back)
    add('numpy', "(e) numpy restatement on the run's own rows", lambda: R.merge_views(h_dets, h_count, np.array(table), 1, **kw))
    add('numpyc', '(e) numpy restatement on the clustered recipe', lambda: R.run(clus, keep_top_k=kw['keep_top_k']))

    r = alternate(legs, a.seconds, a.rounds)
    say()
    for k in legs:
        say('%-86s %9.3f ms   (%.3f .. %.3f)' % (names[k], r[k][0] * 1e3, r[k][1] * 1e3, r[k][2] * 1e3))
    say()
    w = max(r['worst%d' % kw['keep_top_k']][0], r['worst1024'][0])
    say('aim 1: worst-case merge %.3f ms < one forward chunk %.3f ms -> %s (%.1f %% of a chunk)' % (
        w * 1e3, r['chunk'][0] * 1e3, 'MET' if w < r['chunk'][0] else 'MISSED', 100 * w / r['chunk'][0]))
    say('aim 2: merge of the run\'s own rows %.3f ms <= the read-back alone %.3f ms -> %s (%.2fx)' % (
        r['own'][0] * 1e3, r['copy'][0] * 1e3, 'MET' if r['own'][0] <= r['copy'][0] else 'MISSED', r['own'][0] / r['copy'][0]))
    say('finding: the merge is %.2f %% of the whole tiled call; the parent\'s path (copy + numpy, own rows) would take %.3f ms' % (
        100 * r['own'][0] / r['tiled'][0], (r['copy'][0] + r['numpy'][0]) * 1e3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
