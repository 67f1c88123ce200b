"""JPEG encoder timings (ppyolo_hip/jpeg.py JpegEncoder, csrc/jpeg_encode.hip) on the decoded pixels of the two COCO-sized
fixtures of tests/golden/g20_jpeg.npz (500x375 and 640x418) replicated to a batch, at quality 95 and 4:2:0, in ONE process
with the legs alternating:

  stage 1      pixels -> coefficient buffer: one launch, replayed from a captured graph;
  stage 2      coefficient buffer -> entropy-coded bytes + lengths: eight launches, replayed from a captured graph;
  read-back    the lengths, then exactly that many bytes, device -> host (two copies, the first waits for the stream);
  encode()     the whole call, host clock: descriptors, table copy, both stages, read-back, headers; both entropy modes;
  step         the one-lane detection step of the same run: Decode.detect_raw on the same pixels, R50vd-608, one batch at a
               time -- the step an encode of the previous batch's images has to hide behind;
  Pillow       Image.save of the same pixels on the host (libjpeg-turbo, the library cv2.imwrite runs) on 1 thread and on 16.

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.  The condition: stage 1 + stage 2 per batch below the detection step of the same run.

    python tools/jpeg_encode_bench.py [--out profiles/jpeg_encode_bench.txt] [--bs 8] [--seconds 1.0] [--rounds 5] [--no-model]"""
import argparse
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ppyolo_hip.jpeg import JpegDecoder, JpegEncoder  # noqa: E402


def window(fn, seconds):
    """-> seconds per call of fn over a window of at least `seconds` (fn may enqueue; the window ends in a synchronise)."""
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
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(window(fn, seconds))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_encode_bench.txt'))
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_encode_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    files = [g['jpg_' + str(n)].tobytes() for n in g['names'] if str(n).startswith('coco_')]
    two = JpegDecoder().decode(files)
    pixels = [two[i % len(two)].clone() for i in range(a.bs)]
    host_pixels = [t.cpu().numpy() for t in pixels]
    enc, enc_host = JpegEncoder(), JpegEncoder(entropy='host')
    out = enc.encode(pixels)
    assert out == enc_host.encode(pixels), 'the two entropy modes write different files'
    say('%d images (%s), quality %d, %s, restart interval %d; %s; windows >= %.1f s, %d rounds, legs alternating' % (
        a.bs, ', '.join('%dx%d' % (t.shape[1], t.shape[0]) for t in two), enc.quality, enc.subsampling, enc.restart_interval,
        torch.cuda.get_device_name(0), a.seconds, a.rounds))
    say('pixel bytes per batch %d, file bytes per batch %d' % (sum(t.numel() for t in pixels), sum(len(b) for b in out)))

    eb = enc.coefficients(pixels)
    dev_out, lengths = enc.scan_device(eb)
    torch.cuda.synchronize()
    say('coefficient buffer %d bytes, stage 2 workspace %d bytes, output capacity %d bytes, blocks per image %s' % (
        eb.sizes.coef_bytes, eb.sizes.ws_bytes, eb.sizes.out_bytes, sorted(set(int(d.blocks) for d in eb.descs))))
    say()
    from ppyolo_hip import _lib
    L = _lib.lib()
    ws = torch.empty(eb.sizes.ws_bytes, dtype=torch.uint8, device='cuda')

    def stage1():
        _lib.check(L.ppy_jpeg_enc_coefficients(eb.n, eb.descs, eb.table.data_ptr(), eb.coef.data_ptr(), eb.sizes.coef_bytes,
                                               torch.cuda.current_stream().cuda_stream), 'ppy_jpeg_enc_coefficients')

    def stage2():
        _lib.check(L.ppy_jpeg_enc_scan_device(eb.n, eb.descs, eb.table.data_ptr(), eb.coef.data_ptr(), eb.sizes.coef_bytes, dev_out.data_ptr(),
                                              eb.sizes.out_bytes, lengths.data_ptr(), ws.data_ptr(), eb.sizes.ws_bytes,
                                              torch.cuda.current_stream().cuda_stream), 'ppy_jpeg_enc_scan_device')

    def readback():
        lens = lengths.cpu().tolist()
        return dev_out[:sum(lens)].cpu()

    legs = dict(stage1=graph_of(stage1), stage2=graph_of(stage2), readback=readback, encode=lambda: enc.encode(pixels),
                encode_host_entropy=lambda: enc_host.encode(pixels))
    if not a.no_model:
        from conftest import build_model
        from config import PPYOLO_2x_Config
        from model.decode_np import Decode
        cfg = PPYOLO_2x_Config()
        model, _ = build_model(cfg, 0, 'cuda')
        dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
        legs['step'] = lambda: dec.detect_raw(pixels)
    r = alternate(legs, a.seconds, a.rounds)
    names = dict(stage1='stage 1, 1 launch (graph replay)', stage2='stage 2, 8 launches (graph replay)', readback='read-back: lengths, then bytes',
                 encode="encode(), entropy='device'", encode_host_entropy="encode(), entropy='host'",
                 step='one-lane detection step, R50vd-608 bs %d' % a.bs)
    for k in legs:
        say('%-42s %9.3f ms per batch   (%.3f .. %.3f)' % (names[k], r[k][0] * 1e3, r[k][1] * 1e3, r[k][2] * 1e3))
    both = r['stage1'][0] + r['stage2'][0]
    say()
    say('device time of both stages %.3f ms per batch = %.1f images/s' % (both * 1e3, a.bs / both))
    if 'step' in r:
        say('condition: both stages below the one-lane detection step of this run (%.3f ms) -> %s (%.2fx the step)' % (
            r['step'][0] * 1e3, 'MET' if both < r['step'][0] else 'MISSED', both / r['step'][0]))

    # the host baseline: Pillow = libjpeg-turbo, the library behind cv2.imwrite
    try:
        from PIL import Image
    except ImportError:
        say('Pillow is not installed: no host baseline')
    else:
        rgb = [Image.fromarray(np.ascontiguousarray(p[:, :, ::-1])) for p in host_pixels]

        def pil(im):
            bio = io.BytesIO()
            im.save(bio, 'JPEG', quality=enc.quality, subsampling=enc.subsampling)
            return bio.getvalue()
        assert [pil(im) for im in rgb] == out, 'Pillow writes other bytes'
        pool = ThreadPoolExecutor(16)
        rp = alternate({'1': lambda: [pil(im) for im in rgb], '16': lambda: list(pool.map(pil, rgb * 2))}, a.seconds, a.rounds)
        say()
        say('Pillow (libjpeg-turbo) on the host, same pixels, same bytes written:')
        say('  1 thread    %9.3f ms per batch   (%.3f .. %.3f)' % (rp['1'][0] * 1e3, rp['1'][1] * 1e3, rp['1'][2] * 1e3))
        say('  16 threads  %9.3f ms per batch of wall time   (%.3f .. %.3f; two batches per call)' % (
            rp['16'][0] * 1e3 / 2, rp['16'][1] * 1e3 / 2, rp['16'][2] * 1e3 / 2))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
