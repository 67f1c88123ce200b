"""Timings of the Pillow resize (csrc/pil_resize.hip: ppy_preprocess_pil_u8_f32, two launches) beside the cv2-cubic
pre-processing launch it stands next to (csrc/preprocess.hip: ppy_preprocess_u8_f32), in ONE process with the legs alternating:

  (a) cubic, parent   the shipped cv2-cubic launch out of the PARENT commit's library (--parent-lib, a libppyolo_hip.so built
                      from the parent commit), 8 x 480x640 -> 608, replayed from a captured graph;
  (b) cubic, this     the same launch out of this tree's library: it must agree with (a) within the windows' own spread;
  (c) pil, filter f   the new path with each of Pillow's six filters on the same batch, replayed from captured graphs;
  (d) pil, 4K         the same at 8 x 2160x3840 -> 608 with BICUBIC and LANCZOS (39 taps per axis);
  (e) planner         ppy_pil_resize_plan on the host per batch, BICUBIC: 8 equal sizes (2 tables) and 8 distinct sizes (16);
  (f) step            the one-lane detection step of the same run: Decode.detect_raw on the 480x640 batch, R50vd-608.

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.  The condition: (c) BICUBIC takes at most 5 % of (f), so that it hides behind the step as
the decoder's reconstruct stage does, and (e) for 8 distinct sizes stays below (f).  The ratio of (c) BICUBIC to (b) is a
finding, not a condition: Pillow's bicubic reads 5 + 5 taps through an intermediate image where cv2's reads 4 x 4.

    python tools/resize_bench.py [--parent-lib PATH] [--out profiles/pil_resize_bench.txt] [--seconds 1.0] [--rounds 5]"""
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
from ppyolo_hip.preprocess import normalisation_table  # noqa: E402
from ppyolo_hip.resize import BICUBIC, LANCZOS, PilPlanner  # noqa: E402

DISTINCT = [(480, 640), (427, 640), (375, 500), (640, 480), (500, 333), (612, 612), (424, 640), (333, 500)]


def images(sizes, seed):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda() for h, w in sizes]


def cubic_call(fn, imgs, S, lut, out):
    n = len(imgs)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in imgs])
    hs, ws = (ctypes.c_int * n)(*[t.shape[0] for t in imgs]), (ctypes.c_int * n)(*[t.shape[1] for t in imgs])
    st = (ctypes.c_int * n)(*[t.stride(0) for t in imgs])

    def run():
        rc = fn(n, ptrs, hs, ws, st, 1, S, lut.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return run


def pil_call(f, imgs, S, lut, out):
    planner = PilPlanner(f, 'cuda')
    n, h_blob, blob, nbytes, ws = planner.plan(imgs, S, S)
    torch.cuda.synchronize()
    run = lambda: ops.preprocess_pil_images(n, h_blob, blob, nbytes, ws, lut, out, swap_rb=True)      # noqa: E731
    run.keep = planner
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pil_resize_bench.txt'))
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resize_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    S, bs = 608, 8
    from config import PPYOLO_2x_Config
    cfg = PPYOLO_2x_Config()
    nrm = cfg.normalizeImage
    lut = torch.from_numpy(normalisation_table(nrm['mean'], nrm['std'], nrm.get('is_scale', True))).cuda()
    coco, big = images([(480, 640)] * bs, 0), images([(2160, 3840)] * bs, 1)
    out = torch.empty((bs, 3, S, S), dtype=torch.float32, device='cuda')
    say('%d images 640x480 (and 3840x2160) -> %d x %d float32 NCHW; %s; windows >= %.1f s, %d rounds, legs alternating' % (
        bs, S, S, torch.cuda.get_device_name(0), a.seconds, a.rounds))

    legs, names = {}, {}
    this = cubic_call(_lib.lib().ppy_preprocess_u8_f32, coco, S, lut, out)
    this()
    want = out.clone()
    if a.parent_lib:
        P = ctypes.CDLL(os.path.abspath(a.parent_lib))
        P.ppy_preprocess_u8_f32.restype = ctypes.c_int
        P.ppy_preprocess_u8_f32.argtypes = _lib._PROTOS['ppy_preprocess_u8_f32'][1]
        P.ppy_version.restype = ctypes.c_int
        parent = cubic_call(P.ppy_preprocess_u8_f32, coco, S, lut, out)
        out.zero_()
        parent()
        say('parent library: ppy_version %d (this tree: %d); its cubic launch writes the same bits as this tree\'s: %s' % (
            P.ppy_version(), _lib.lib().ppy_version(), torch.equal(out.view(torch.int32), want.view(torch.int32))))
        legs['cubic_parent'], names['cubic_parent'] = graph_of(parent), '(a) cv2 cubic, parent library, 1 launch'
    else:
        say('no --parent-lib given: leg (a) is not measured')
    legs['cubic_this'], names['cubic_this'] = graph_of(this), '(b) cv2 cubic, this library, 1 launch'
    keep = []
    for f in range(6):
        run = pil_call(f, coco, S, lut, out)
        keep.append(run)
        legs['pil%d' % f], names['pil%d' % f] = graph_of(run), '(c) pil %-8s 640x480, 2 launches' % _lib.PIL_FILTERS[f]
    for f in (BICUBIC, LANCZOS):
        run = pil_call(f, big, S, lut, out)
        keep.append(run)
        legs['big%d' % f], names['big%d' % f] = graph_of(run), '(d) pil %-8s 3840x2160, 2 launches' % _lib.PIL_FILTERS[f]

    stage = np.zeros(1 << 20, np.int64)
    for key, sizes, label in (('plan_equal', [(480, 640)] * bs, '8 equal sizes'), ('plan_distinct', DISTINCT, '8 distinct sizes')):
        descs = [(8, 3 * w, h, w) for h, w in sizes]
        legs[key] = lambda d=descs: ops.pil_resize_plan(d, S, S, BICUBIC, lambda nbytes: stage.ctypes.data)
        nbytes, _ = legs[key]()
        assert nbytes <= stage.nbytes
        names[key] = '(e) host planner, bicubic, %s (%d KB)' % (label, nbytes >> 10)

    if not a.no_model:
        from conftest import build_model
        from model.decode_np import Decode
        model, _ = build_model(cfg, 0, 'cuda')
        dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
        legs['step'], names['step'] = (lambda: dec.detect_raw(coco)), '(f) one-lane detection step, R50vd-608 bs %d' % bs

    r = alternate(legs, a.seconds, a.rounds)
    say()
    for k in legs:
        say('%-52s %9.3f ms per batch   (%.3f .. %.3f)' % (names[k], r[k][0] * 1e3, r[k][1] * 1e3, r[k][2] * 1e3))
    say()
    bic, cub = r['pil%d' % BICUBIC], r['cubic_this']
    say('finding: pil bicubic / cv2 cubic (this library) = %.2fx' % (bic[0] / cub[0]))
    if 'cubic_parent' in r:
        par = r['cubic_parent']
        apart = cub[1] > par[2] or par[1] > cub[2]
        say('parent unchanged: cubic %.4f ms (%.4f .. %.4f) here, %.4f ms (%.4f .. %.4f) from the parent library -> %s' % (
            cub[0] * 1e3, cub[1] * 1e3, cub[2] * 1e3, par[0] * 1e3, par[1] * 1e3, par[2] * 1e3,
            'the windows do NOT overlap: a finding' if apart else 'within the windows\' own spread'))
    if 'step' in r:
        step = r['step'][0]
        say('condition 1: pil bicubic %.3f ms <= 5 %% of the step %.3f ms (= %.3f ms) -> %s (%.1f %%)' % (
            bic[0] * 1e3, step * 1e3, 0.05 * step * 1e3, 'MET' if bic[0] <= 0.05 * step else 'MISSED', 100 * bic[0] / step))
        pd = r['plan_distinct'][0]
        say('condition 2: host planner, 8 distinct sizes %.3f ms < the step %.3f ms -> %s (%.1f %%)' % (
            pd * 1e3, step * 1e3, 'MET' if pd < step else 'MISSED', 100 * pd / step))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
