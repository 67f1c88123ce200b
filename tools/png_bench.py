"""PNG decoder timings (ppyolo_hip/png.py PngDecoder, csrc/png.hip) on the decoded pixels of the two COCO-sized fixtures of
tests/golden/g20_jpeg.npz (500x375 and 640x418), written as PNG by Pillow at its defaults (libpng's adaptive filters) and
replicated to a batch of 8, in ONE process with the legs alternating:

  (a) host stage   chunk walk + CRCs + inflate + filter-byte check + the copy into the pinned buffer: per image on 1 thread,
                   and the wall time of the batch on 16 threads; beside Pillow's whole decode (Image.open().convert('RGB'))
                   of the same files on 1 thread and on 16;
  (b) copy         [descriptor table | scanline streams] host -> device out of the pinned buffer;
  (c) reconstruct  ppy_png_reconstruct_u8 per batch, replayed from a captured graph;
  (d) filters      (c) on an all-Paeth file, an all-None file and an Adam7 file of the same pixels (tests/png_synth.py);
  (e) 4K           (c) on one 3840x2160 image (the same pixels tiled, written by Pillow);
  (f) step         the one-lane detection step of the same run: Decode.detect_raw on the batch, R50vd-608;
  (g) files        Decode.detect_files(files, decoder=ImageDecoder()) on the PNG batch and on the JPEG batch, host clock.

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.  Conditions: (c) takes at most 5 % of (f); the host stage on one thread is not slower than
Pillow's whole decode of the same file.  Whether the host stage scales over the pool's threads is a finding.

    python tools/png_bench.py [--out profiles/png_bench.txt] [--bs 8] [--seconds 1.0] [--rounds 5] [--no-model]"""
import argparse
import ctypes
import io
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from jpeg_encode_bench import alternate, graph_of  # noqa: E402
from ppyolo_hip import _lib  # noqa: E402
from ppyolo_hip.imagefile import ImageDecoder  # noqa: E402
from ppyolo_hip.jpeg import JpegDecoder  # noqa: E402
from ppyolo_hip.png import PngDecoder  # noqa: E402


def pillow_png(bgr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, 'PNG')
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def reconstruct_call(dec, files):
    """The launches alone on a resident blob, as a C caller enqueues them -> (run, outputs, keep-alive)."""
    L = _lib.lib()
    hb = dec.host_decode(files)
    n = hb.n
    outs = [torch.empty((h, w, 3), dtype=torch.uint8, device='cuda') for h, w in hb.sizes]
    _lib.check(L.ppy_png_pack_table(n, hb.descs, (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs]),
                                    (ctypes.c_longlong * n)(*[t.stride(0) for t in outs]), hb.stage.data_ptr(), hb.table_bytes))
    blob = hb.stage[:hb.total_bytes].cuda()
    dec.release(hb)
    ws_bytes = L.ppy_png_workspace_bytes(n, hb.descs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')

    def run():
        _lib.check(L.ppy_png_reconstruct_u8(n, hb.descs, blob.data_ptr(), blob.data_ptr() + hb.table_bytes, hb.total_bytes - hb.table_bytes,
                                            ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream), 'ppy_png_reconstruct_u8')
    return run, outs, (hb, blob, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_bench.txt'))
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('png_bench needs the MI355X: a time taken anywhere else says nothing')
    import png_synth as S
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    jpegs = [g['jpg_' + str(n)].tobytes() for n in g['names'] if str(n).startswith('coco_')]
    two = [t.cpu().numpy() for t in JpegDecoder().decode(jpegs)]
    pngs = [pillow_png(px) for px in two]
    files = [pngs[i % len(pngs)] for i in range(a.bs)]
    jfiles = [jpegs[i % len(jpegs)] for i in range(a.bs)]
    pixels = [two[i % len(two)] for i in range(a.bs)]
    dec = PngDecoder()
    got = dec.decode(files)
    assert all(np.array_equal(t.cpu().numpy(), px) for t, px in zip(got, pixels)), 'the decoder does not return the pixels Pillow wrote'
    say('%d PNG files (%s; %s bytes), Pillow defaults; %s; windows >= %.1f s, %d rounds, legs alternating' % (
        a.bs, ', '.join('%dx%d' % (px.shape[1], px.shape[0]) for px in two), ' and '.join(str(len(p)) for p in pngs),
        torch.cuda.get_device_name(0), a.seconds, a.rounds))
    hb = dec.host_decode(files)
    say('pixel bytes per batch %d, file bytes per batch %d, staged bytes per batch %d' % (
        sum(px.size for px in pixels), sum(len(f) for f in files), hb.total_bytes))
    dec.release(hb)

    legs, names, keep = {}, {}, []
    late = {}
    if not a.no_model:
        from conftest import build_model
        from config import PPYOLO_2x_Config
        from model.decode_np import Decode
        cfg = PPYOLO_2x_Config()
        model, _ = build_model(cfg, 0, 'cuda')
        det = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
        dev = [torch.from_numpy(px).cuda() for px in pixels]
        both = ImageDecoder()
        det.detect_raw(dev)      # the plan is built before any graph of this tool is captured: built after them, its first run
                                 # ended in ppy_conv3x3_conv1x1_f32 'bad argument' (seen once on the MI355X; cause not found)
        late['step'], names['step'] = (lambda: det.detect_raw(dev)), '(f) one-lane detection step, R50vd-608 bs %d' % a.bs
        late['files_png'], names['files_png'] = (lambda: det.detect_files(files, decoder=both)), '(g) detect_files, PNG batch, ImageDecoder'
        late['files_jpg'], names['files_jpg'] = (lambda: det.detect_files(jfiles, decoder=both)), '(g) detect_files, JPEG batch, ImageDecoder'

    one, pool_dec = PngDecoder(threads=1), PngDecoder(threads=16)

    def host(d):
        def run():
            d.release(d.host_decode(files))
        return run
    legs['host1'], names['host1'] = host(one), '(a) host stage, batch of %d on 1 thread' % a.bs
    legs['host16'], names['host16'] = host(pool_dec), '(a) host stage, batch of %d on 16 threads' % a.bs
    pool = ThreadPoolExecutor(max_workers=16)
    legs['pil1'], names['pil1'] = (lambda: [pillow_decode(f) for f in files]), '(a) Pillow whole decode, batch on 1 thread'
    legs['pil16'], names['pil16'] = (lambda: list(pool.map(pillow_decode, files))), '(a) Pillow whole decode, batch on 16 threads'

    hb = dec.host_decode(files)
    blob = torch.empty(hb.total_bytes, dtype=torch.uint8, device='cuda')
    stage, total = hb.stage, hb.total_bytes
    legs['h2d'], names['h2d'] = (lambda: blob.copy_(stage[:total], non_blocking=True)), '(b) host -> device copy, %d bytes' % total
    dec.release(hb)

    run, outs, k = reconstruct_call(PngDecoder(), files)
    keep.append(k)
    run()
    assert all(np.array_equal(t.cpu().numpy(), px) for t, px in zip(outs, pixels))
    legs['recon'], names['recon'] = graph_of(run), '(c) reconstruct, adaptive filters (Pillow), 1 launch'
    variants = (('paeth', 'all Paeth', dict(filters=4)), ('none', 'all None', dict(filters=0)), ('adam7', 'Adam7, filters cycling', dict(filters=[0, 1, 2, 3, 4], interlace=1)))
    for key, label, kw in variants:
        synth = [S.make_png(px[..., ::-1].astype(np.int64), 2, 8, **kw) for px in two]
        run, outs, k = reconstruct_call(PngDecoder(), [synth[i % len(synth)] for i in range(a.bs)])
        keep.append(k)
        run()
        assert all(np.array_equal(t.cpu().numpy(), px) for t, px in zip(outs, pixels)), key
        legs[key], names[key] = graph_of(run), '(d) reconstruct, %s' % label
    big = np.tile(two[-1], (6, 6, 1))[:2160, :3840]
    run, outs, k = reconstruct_call(PngDecoder(), [pillow_png(big)])
    keep.append(k)
    run()
    assert np.array_equal(outs[0].cpu().numpy(), big)
    legs['4k'], names['4k'] = graph_of(run), '(e) reconstruct, one 3840x2160 image'

    legs.update(late)                       # printed in the order of the legs' letters
    r = alternate(legs, a.seconds, a.rounds)
    say()
    for key in legs:
        say('%-58s %9.3f ms per batch   (%.3f .. %.3f)' % (names[key], r[key][0] * 1e3, r[key][1] * 1e3, r[key][2] * 1e3))
    say()
    h1, h16, p1, p16 = r['host1'][0], r['host16'][0], r['pil1'][0], r['pil16'][0]
    say('host stage per image on 1 thread %.3f ms; Pillow whole decode per image on 1 thread %.3f ms' % (h1 / a.bs * 1e3, p1 / a.bs * 1e3))
    say('condition 2: host stage on one thread %.3f ms <= Pillow whole decode %.3f ms per batch -> %s (%.2fx)' % (
        h1 * 1e3, p1 * 1e3, 'MET' if h1 <= p1 else 'MISSED', h1 / p1))
    say('finding: 16 threads over 1 thread: host stage %.2fx faster, Pillow %.2fx faster (%d images; 16 CPUs)' % (h1 / h16, p1 / p16, a.bs))
    if 'step' in r:
        step, rec = r['step'][0], r['recon'][0]
        say('condition 1: reconstruct %.3f ms <= 5 %% of the step %.3f ms (= %.3f ms) -> %s (%.1f %%)' % (
            rec * 1e3, step * 1e3, 0.05 * step * 1e3, 'MET' if rec <= 0.05 * step else 'MISSED', 100 * rec / step))
        say('finding: detect_files on PNG / on JPEG = %.2fx' % (r['files_png'][0] / r['files_jpg'][0]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
