"""Timings of the detection crops (csrc/pil_crop.hip: ppy_pil_crop_rows_u8, four launches, boxes read on the device) beside the
same pixel work done the only way the parent commit could do it, in ONE process with the legs alternating:

  (a) crop, filter f    the new call: 8 images 640x480, 100 rows per image with uniform integer boxes -> 800 crops of
                        128 x 128, replayed from a captured graph;
  (b) resize, filter f  PilResizer's launches (ppy_pil_resize_u8 out of --parent-lib, a libppyolo_hip.so built from the PARENT
                        commit; without it this tree's library, whose pil_resize.hip is the parent's) on the same 800 crops
                        handed over as pre-cut views `image[y0:y1, x0:x1]`: host-planned tables, two launches, replayed from a
                        captured graph.  Integer boxes make the two legs read the same taps (not the same pixels at the box
                        edges: a view ends where the box ends, a crop reads on);
  (p) planner           ppy_pil_resize_plan on the host for those 800 views, BICUBIC: the time (b) needs before it can launch
                        and (a) does not have -- reported separately;
  (c) step              the one-lane detection step of the same run: Decode.detect_raw on the 640x480 batch, R50vd-608.

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.  The aim: (a) takes at most 1.5 x (b) per filter -- (a) adds two latency-sized launches and
per-crop tables that (b) shares between images.  (a) / (c) is a finding.

    python tools/crop_bench.py [--parent-lib PATH] [--out profiles/crop_bench.txt] [--seconds 1.0] [--rounds 5]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from jpeg_encode_bench import alternate, graph_of  # noqa: E402
from ppyolo_hip import _lib, ops  # noqa: E402
from ppyolo_hip.crops import CropLauncher  # noqa: E402
from ppyolo_hip.resize import BICUBIC, PilPlanner  # noqa: E402

H, W, BS, K, OW, OH = 480, 640, 8, 100, 128, 128


def rows(seed):
    """[BS, K, 6] float32: class 0, score 0.9, integer boxes with uniform corners, at least one pixel wide."""
    rng = np.random.RandomState(seed)
    d = np.zeros((BS, K, 6), np.float32)
    d[:, :, 1] = 0.9
    xs = np.sort(rng.randint(0, W + 1, (BS, K, 2)), axis=2)
    ys = np.sort(rng.randint(0, H + 1, (BS, K, 2)), axis=2)
    xs[:, :, 1] = np.maximum(xs[:, :, 1], xs[:, :, 0] + 1)
    ys[:, :, 1] = np.maximum(ys[:, :, 1], ys[:, :, 0] + 1)
    xs[:, :, 0] -= xs[:, :, 1] > W
    ys[:, :, 0] -= ys[:, :, 1] > H
    d[:, :, 2], d[:, :, 4] = xs[:, :, 0], np.minimum(xs[:, :, 1], W)
    d[:, :, 3], d[:, :, 5] = ys[:, :, 0], np.minimum(ys[:, :, 1], H)
    return d


def crop_call(f, imgs, dets, count):
    launcher = CropLauncher(f, 'cuda')
    descs, d_images, ws, out, src, total, boxes = launcher.prepare(imgs, 0, K, OW, OH, 0.0, K)
    torch.cuda.synchronize()
    run = lambda: ops.pil_crop_rows_u8(descs, d_images, dets, count, 0.0, 0.0, K, OW, OH, f, ws, out, src, total, boxes)      # noqa: E731
    run.keep, run.out, run.total = launcher, out, total
    return run


def resize_call(fn, f, views):
    planner = PilPlanner(f, 'cuda')
    n, h_blob, blob, nbytes, ws = planner.plan(views, OW, OH)
    out = torch.empty((n, OH, OW, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    wp, wn = (0, 0) if ws is None else (ws.data_ptr(), ws.numel())

    def run():
        rc = fn(n, h_blob, blob.data_ptr(), nbytes, wp, wn, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    run.keep, run.out = planner, out
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'crop_bench.txt'))
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('crop_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(0)
    host = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(BS)]
    imgs = [torch.from_numpy(im).cuda() for im in host]
    d = rows(1)
    dets, count = torch.from_numpy(d).cuda(), torch.full((BS,), K, dtype=torch.int32, device='cuda')
    views = [imgs[i][int(r[3]):int(r[5]), int(r[2]):int(r[4])] for i in range(BS) for r in d[i]]
    say('%d images %dx%d, %d rows each with uniform integer boxes -> %d crops of %d x %d uint8; %s; windows >= %.1f s, %d rounds, '
        'legs alternating' % (BS, W, H, K, BS * K, OW, OH, torch.cuda.get_device_name(0), a.seconds, a.rounds))

    resize_fn = _lib.lib().ppy_pil_resize_u8
    if a.parent_lib:
        P = ctypes.CDLL(os.path.abspath(a.parent_lib))
        P.ppy_pil_resize_u8.restype = ctypes.c_int
        P.ppy_pil_resize_u8.argtypes = _lib._PROTOS['ppy_pil_resize_u8'][1]
        P.ppy_version.restype = ctypes.c_int
        resize_fn = P.ppy_pil_resize_u8
        say('leg (b) launches out of the parent library (ppy_version %d; this tree: %d)' % (P.ppy_version(), _lib.lib().ppy_version()))
    else:
        say('no --parent-lib given: leg (b) launches out of this tree\'s library (its pil_resize.hip is the parent\'s)')

    legs, names, keep = {}, {}, []
    for f in range(6):
        ca, rb = crop_call(f, imgs, dets, count), resize_call(resize_fn, f, views)
        ca()
        rb()
        torch.cuda.synchronize()
        assert int(ca.total.cpu()[0]) == BS * K
        if a.parent_lib:          # the parent's launch and this tree's write the same bits
            mine = resize_call(_lib.lib().ppy_pil_resize_u8, f, views)
            mine()
            assert torch.equal(mine.out, rb.out), 'ppy_pil_resize_u8 of this tree differs from the parent library'
        same = (ca.out == rb.out).flatten(1).all(1).sum().item()
        say('%-8s crops equal to the resize of their pre-cut view: %d of %d (a crop reads past its box, a view cannot)' % (
            _lib.PIL_FILTERS[f], same, BS * K))
        keep += [ca, rb]
        legs['crop%d' % f], names['crop%d' % f] = graph_of(ca), '(a) crop   %-8s 4 launches' % _lib.PIL_FILTERS[f]
        legs['view%d' % f], names['view%d' % f] = graph_of(rb), '(b) resize %-8s of 800 views, 2 launches' % _lib.PIL_FILTERS[f]

    stage = np.zeros(1 << 22, np.int64)
    descs = [(t.data_ptr(), max(t.stride(0), 3 * t.shape[1]), t.shape[0], t.shape[1]) for t in views]
    legs['plan'] = lambda: ops.pil_resize_plan(descs, OW, OH, BICUBIC, lambda nbytes: stage.ctypes.data)
    nbytes, _ = legs['plan']()
    assert nbytes <= stage.nbytes
    names['plan'] = '(p) host planner of (b), bicubic, 800 views (%d KB)' % (nbytes >> 10)

    if not a.no_model:
        from config import PPYOLO_2x_Config
        from conftest import build_model
        from model.decode_np import Decode
        cfg = PPYOLO_2x_Config()
        model, _ = build_model(cfg, 0, 'cuda')
        dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
        legs['step'], names['step'] = (lambda: dec.detect_raw(imgs)), '(c) one-lane detection step, R50vd-608 bs %d' % BS

    r = alternate(legs, a.seconds, a.rounds)
    say()
    for k in legs:
        say('%-52s %9.3f ms per batch   (%.3f .. %.3f)' % (names[k], r[k][0] * 1e3, r[k][1] * 1e3, r[k][2] * 1e3))
    say()
    for f in range(6):
        ca, rb = r['crop%d' % f], r['view%d' % f]
        line = 'aim, %-8s: crop %.3f ms <= 1.5 x resize of views %.3f ms (= %.3f ms) -> %s (%.2fx)' % (
            _lib.PIL_FILTERS[f], ca[0] * 1e3, rb[0] * 1e3, 1.5 * rb[0] * 1e3, 'MET' if ca[0] <= 1.5 * rb[0] else 'MISSED', ca[0] / rb[0])
        if 'step' in r:
            line += '; finding: crop / step = %.1f %%' % (100 * ca[0] / r['step'][0])
        say(line)
    say('the planner (p) is host time leg (b) spends per batch before its launches and leg (a) does not: %.3f ms' % (r['plan'][0] * 1e3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
