"""JPEG decoder timings (ppyolo_hip/jpeg.py, csrc/jpeg.hip).

    python tools/jpeg_bench.py [--bs 8] [--window 1.0] [--rounds 5] [--no-model] [--entropy {host,device}]

Input: the COCO-sized files of tests/golden/g20_jpeg.npz replicated to a batch.  Reports
  entropy_ms_per_image   host stage (parse + Huffman) at 1 and 16 threads, wall clock over 4 batches per call;
  h2d                    bytes and time (device events) of the one copy per batch: descriptor table + coefficients;
  reconstruct            the two kernels as the mean of graph-replayed launches, beside a device-to-device copy moving the
                         same number of bytes (coefficients read + pixels written), replayed the same way: the roofline;
  detect                 files -> detections images/s at R50vd-608 with the decoder on a producer thread and a stream of its
                         own, one batch ahead, beside detect_raw on the same images already decoded, alternating in one run;
                         and, to attribute a gap, detect_raw beside the entropy stage alone and beside copy + kernels alone;
  pillow_ms_per_image    Pillow's (libjpeg-turbo's) decode of the same files at 1 and 16 threads, where Pillow is installed.
--entropy device adds the device entropy mode (JpegDecoder(entropy='device'), csrc/jpeg_entropy.hip) to the same run:
  device_entropy         prepass_ms_per_image: the host marker pass at 1 and 16 threads; h2d: bytes and time of its one copy
                         (table + plan + compressed scan records); entropy_ms: the entropy launches of a batch replayed from a
                         graph, per subsequence size, beside reconstruct.ms; link_fixed: subsequences the cross-workgroup step
                         repaired; and in detect the legs files_device (status read back per batch) and files_device_nocheck.
--progressive [--parent-lib PATH] runs, instead of all the above, the legs of the files JpegDecoder(accept='all') adds:
  host_ms_per_image      the host stage at 1 and 16 threads on the progressive COCO-sized goldens (g22_jpeg_full.npz), on
                         baseline files of the same pixels (default decoder, and accept='all'), and Pillow's whole decode;
  reconstruct_ms         the two launches on a batch of 480x640 4:2:0 / 4:4:0 / 4:1:1 images, --rounds windows each, alternating;
  baseline_reconstruct_ms  the two launches on the baseline batch, this library against the one at PATH (the parent commit's
                         build), both loaded into this process, --rounds alternating windows.
Every timed window lasts at least --window seconds (the repeat count is calibrated first); the detect legs alternate for
--rounds rounds and report every round, so the spread is in the output.  One JSON line."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests')]

from ppyolo_hip import _lib  # noqa: E402
from ppyolo_hip.jpeg import JpegDecoder  # noqa: E402


def files(bs):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    big = [g['jpg_' + str(n)].tobytes() for n in g['names'] if str(n).startswith('coco_')]
    return [big[i % len(big)] for i in range(bs)]


def wall_s(fn, window):
    """Seconds per call of a host function, over at least `window` seconds."""
    fn()
    n, t0 = 0, time.perf_counter()
    while n < 3 or time.perf_counter() - t0 < window:
        fn()
        n += 1
    return (time.perf_counter() - t0) / n


def event_ms(fn, window):
    """Device time per call of `fn` (events around a loop that lasts at least `window` seconds)."""
    def run(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters
    fn()
    torch.cuda.synchronize()
    one = max(run(50), 1e-4)
    return run(max(int(window * 1e3 / one), 50))


def replay_ms(fn, window):
    """Mean time of `fn`'s launches replayed from a captured graph."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return event_ms(g.replay, window)


def progressive_legs(a):
    """--progressive: the files JpegDecoder(accept='all') adds.  (a) host stage per image on the progressive COCO-sized goldens
    beside baseline files of the same pixels and Pillow's whole decode; (b) the two reconstruct launches on 4:4:0, 4:1:1 and
    4:2:0 images of one size; (c) the two launches on the baseline batch, this library against --parent-lib, alternating."""
    import ctypes

    import jpeg_full_fixtures as FF
    import jpeg_full_synth as FS
    import jpeg_synth as S
    L = _lib.lib()
    res = dict(bs=a.bs, device=torch.cuda.get_device_name(0))
    prog = [FF.data(n) for n in FF.names() if '_coco_' in n]
    try:
        from PIL import Image
    except ImportError:
        Image = None
        base, res['baseline_files'] = files(len(prog)), 'the originals (no Pillow to re-encode them)'
    else:
        def again(b):
            bio = io.BytesIO()
            Image.fromarray(np.asarray(Image.open(io.BytesIO(b)).convert('RGB'))).save(bio, 'JPEG', quality=75, subsampling=2)
            return bio.getvalue()
        base, res['baseline_files'] = [again(b) for b in files(len(prog))], 'Pillow, quality 75, 4:2:0, as the progressive ones'
    res['file_bytes'] = dict(progressive=sum(map(len, prog)), baseline=sum(map(len, base)))
    host = {}
    for key, data, accept in (('progressive', prog, 'all'), ('baseline', base, 'baseline'), ('baseline_accept_all', base, 'all')):
        host[key] = {}
        for th in (1, 16):
            jd = JpegDecoder(threads=th, accept=accept)
            many = [data[i % len(data)] for i in range(4 * a.bs)]
            host[key][str(th)] = wall_s(lambda: jd.release(jd.entropy_decode(many)), a.window) * 1e3 / len(many)
    if Image is not None:
        host['pillow_progressive'] = {}
        for th in (1, 16):
            pool = ThreadPoolExecutor(th)
            many = [prog[i % len(prog)] for i in range(4 * a.bs)]
            host['pillow_progressive'][str(th)] = wall_s(
                lambda: list(pool.map(lambda b: np.asarray(Image.open(io.BytesIO(b)).convert('RGB')), many)), a.window) * 1e3 / len(many)
            pool.shutdown()
    res['host_ms_per_image'] = host

    def launches(lib, hb, blob, ws):
        coef_bytes = hb.total_bytes - hb.table_bytes

        def run():
            _lib.check(lib.ppy_jpeg_reconstruct_u8(hb.n, hb.descs, 1, blob.data_ptr(), blob.data_ptr() + hb.table_bytes, coef_bytes,
                                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), 'ppy_jpeg_reconstruct_u8')
        return run

    # (b) one batch per sampling, all in one run
    jd = JpegDecoder(accept='all')
    rng = np.random.default_rng(7)
    res['reconstruct_ms'] = {}
    keep = []
    for name, luma in (('420', (2, 2)), ('440', (1, 2)), ('411', (4, 1))):
        one = S.encode(FS.synth(rng, 480, 640, luma))
        hb = jd.entropy_decode([one] * a.bs)
        outs = jd.reconstruct(hb)
        blob = torch.empty(hb.total_bytes, dtype=torch.uint8, device='cuda')
        blob.copy_(hb.stage[:hb.total_bytes])
        torch.cuda.synchronize()
        ws = torch.empty(L.ppy_jpeg_workspace_bytes(hb.n, hb.descs), dtype=torch.uint8, device='cuda')
        keep.append((name, launches(L, hb, blob, ws), outs))
    for _ in range(a.rounds):
        for name, run, _ in keep:
            res['reconstruct_ms'].setdefault(name, []).append(round(replay_ms(run, a.window), 5))

    # (c) the baseline batch: this library against the parent's
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        for fn in ('ppy_jpeg_pack_table', 'ppy_jpeg_reconstruct_u8'):
            getattr(parent, fn).restype, getattr(parent, fn).argtypes = _lib._PROTOS[fn]
        jd0 = JpegDecoder()
        hb = jd0.entropy_decode(files(a.bs))
        outs = jd0.reconstruct(hb)              # packs this library's table into the staging buffer
        torch.cuda.synchronize()
        ws = torch.empty(L.ppy_jpeg_workspace_bytes(hb.n, hb.descs), dtype=torch.uint8, device='cuda')
        legs = []
        for key, lib in (('this', L), ('parent', parent)):
            stage = hb.stage[:hb.total_bytes].clone()
            _lib.check(lib.ppy_jpeg_pack_table(hb.n, hb.descs, (ctypes.c_void_p * hb.n)(*[t.data_ptr() for t in outs]),
                                               (ctypes.c_longlong * hb.n)(*[3 * t.shape[1] for t in outs]), 1, stage.data_ptr(), hb.table_bytes),
                       'ppy_jpeg_pack_table')
            legs.append((key, launches(lib, hb, stage.cuda(), ws)))
        ab = {'this': [], 'parent': []}
        for _ in range(a.rounds):
            for key, run in legs:
                ab[key].append(round(replay_ms(run, a.window), 5))
        res['baseline_reconstruct_ms'] = ab
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--entropy', choices=('host', 'device'), default='host')
    ap.add_argument('--progressive', action='store_true', help='only the legs of the files accept= adds (progressive_legs)')
    ap.add_argument('--parent-lib', default=None, help="--progressive: the parent commit's libppyolo_hip.so for the A/B leg")
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a ROCm device'
    if a.progressive:
        return progressive_legs(a)
    data = files(a.bs)
    L = _lib.lib()
    res = dict(bs=a.bs, device=torch.cuda.get_device_name(0), file_bytes=sum(len(d) for d in data))

    # host stage
    res['entropy_ms_per_image'] = {}
    for th in (1, 16):
        jd = JpegDecoder(threads=th)
        many = data * 4
        res['entropy_ms_per_image'][str(th)] = wall_s(lambda: jd.release(jd.entropy_decode(many)), a.window) * 1e3 / len(many)

    # copy + kernels
    jd = JpegDecoder()
    hb = jd.entropy_decode(data)
    outs = jd.reconstruct(hb)
    torch.cuda.synchronize()
    pixel_bytes = sum(t.numel() for t in outs)
    coef_bytes = hb.total_bytes - hb.table_bytes
    blob = torch.empty(hb.total_bytes, dtype=torch.uint8, device='cuda')
    res['h2d'] = dict(bytes=hb.total_bytes, ms=event_ms(lambda: blob.copy_(hb.stage[:hb.total_bytes], non_blocking=True), a.window))
    ws_bytes = L.ppy_jpeg_workspace_bytes(hb.n, hb.descs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')

    def kernels():
        _lib.check(L.ppy_jpeg_reconstruct_u8(hb.n, hb.descs, 1, blob.data_ptr(), blob.data_ptr() + hb.table_bytes, coef_bytes, ws.data_ptr(),
                                             ws_bytes, torch.cuda.current_stream().cuda_stream), 'ppy_jpeg_reconstruct_u8')
    half = (coef_bytes + pixel_bytes) // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device='cuda'), torch.empty(half, dtype=torch.uint8, device='cuda')
    k_ms, c_ms = replay_ms(kernels, a.window), replay_ms(lambda: dst.copy_(src), a.window)
    res['reconstruct'] = dict(ms=k_ms, coef_bytes=coef_bytes, pixel_bytes=pixel_bytes, plane_bytes=ws_bytes,
                              copy_same_bytes_ms=c_ms, images_per_s=a.bs / k_ms * 1e3)

    # the device entropy mode: marker pass, copy, entropy launches
    if a.entropy == 'device':
        import ctypes
        de = dict(prepass_ms_per_image={})
        for th in (1, 16):
            jdp = JpegDecoder(threads=th, entropy='device')
            many = data * 4
            de['prepass_ms_per_image'][str(th)] = wall_s(lambda: jdp.release(jdp.entropy_decode(many)), a.window) * 1e3 / len(many)
        jde = JpegDecoder(entropy='device')
        hbd = jde.entropy_decode(data)
        outs_d = jde.reconstruct(hbd)
        assert all(torch.equal(x, y) for x, y in zip(outs, outs_d)), 'device entropy mode decodes other pixels'
        blob_d = torch.empty(hbd.total_bytes, dtype=torch.uint8, device='cuda')
        de['h2d'] = dict(bytes=hbd.total_bytes, ms=event_ms(lambda: blob_d.copy_(hbd.stage[:hbd.total_bytes], non_blocking=True), a.window))
        h_plan = hbd.stage.data_ptr() + hbd.table_bytes
        coef_d = torch.empty(hbd.coef_bytes, dtype=torch.uint8, device='cuda')
        status = torch.empty((3, hbd.n), dtype=torch.int32, device='cuda')
        de['entropy_ms'], de['link_fixed'], de['subsequences'] = {}, {}, {}
        for sub in (8, 16, 32, 64, 128, 256, 1024):
            wsb = ctypes.c_size_t()
            _lib.check(L.ppy_jpeg_entropy_plan(hbd.n, hbd.descs, h_plan + hbd.plan_bytes, hbd.scan_bytes, (ctypes.c_longlong * hbd.n)(*hbd.scan_off),
                                               sub, h_plan, hbd.plan_bytes, ctypes.byref(wsb)), 'ppy_jpeg_entropy_plan')
            blob_d.copy_(hbd.stage[:hbd.total_bytes])
            torch.cuda.synchronize()
            ews = torch.empty(max(wsb.value, 16), dtype=torch.uint8, device='cuda')

            def entropy():
                _lib.check(L.ppy_jpeg_entropy_device(hbd.n, h_plan, blob_d.data_ptr() + hbd.table_bytes,
                                                     blob_d.data_ptr() + hbd.table_bytes + hbd.plan_bytes, sub, coef_d.data_ptr(), hbd.coef_bytes,
                                                     status.data_ptr(), ews.data_ptr(), wsb.value, torch.cuda.current_stream().cuda_stream),
                           'ppy_jpeg_entropy_device')
            de['entropy_ms'][str(sub)] = replay_ms(entropy, a.window / 4)
            assert not status[:2].any().item()
            de['link_fixed'][str(sub)] = int(status[2].sum().item())
            de['subsequences'][str(sub)] = wsb.value // 24
        jde.release(hbd)
        res['device_entropy'] = de

    # files -> detections, beside pre-decoded pixels -> detections
    if not a.no_model:
        from conftest import build_model
        from config import PPYOLO_2x_Config
        from model.decode_np import Decode
        cfg = PPYOLO_2x_Config()
        model, _ = build_model(cfg, 0, 'cuda')
        dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
        pixels = [t.clone() for t in outs]
        producer = ThreadPoolExecutor(1)

        def raw_fed(n):
            for _ in range(n):
                dec.detect_raw(pixels)

        side = torch.cuda.Stream()
        jd_dev = JpegDecoder()
        fixed = jd_dev.entropy_decode(data)   # (a decoder of its own: nothing else writes its staging buffer)

        def produce_all():                    # the whole decode, one batch ahead, on a stream of its own
            with torch.cuda.stream(side):
                imgs = jd.decode(data)
                ev = torch.cuda.Event()
                ev.record(side)
            return imgs, ev

        def produce_host_only():              # attribution: the entropy stage alone beside the model (its output is dropped)
            jd_host.release(jd_host.entropy_decode(data))
            return pixels, None

        def produce_device_only():            # attribution: copy + kernels alone, from one fixed host batch
            with torch.cuda.stream(side):
                imgs = jd_dev.reconstruct(fixed)
                ev = torch.cuda.Event()
                ev.record(side)
            return imgs, ev

        def fed(produce):
            def run(n):
                fut = producer.submit(produce)
                for _ in range(n):
                    imgs, ev = fut.result()
                    fut = producer.submit(produce)
                    if ev is not None:
                        torch.cuda.current_stream().wait_event(ev)
                    dec.detect_raw(imgs)      # ends in a host synchronise, so imgs are free when they are dropped
                fut.result()
                torch.cuda.synchronize()
            return run
        jd_host = JpegDecoder()
        legs = [('raw', raw_fed), ('files', fed(produce_all)), ('raw_beside_entropy_stage', fed(produce_host_only)),
                ('raw_beside_copy_and_kernels', fed(produce_device_only))]
        if a.entropy == 'device':
            jd_e = JpegDecoder(entropy='device')

            def produce_device_entropy(check):
                def produce():
                    with torch.cuda.stream(side):
                        imgs = jd_e.decode(data, check=check)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    return imgs, ev
                return produce
            legs += [('files_device', fed(produce_device_entropy(True))), ('files_device_nocheck', fed(produce_device_entropy(False)))]
        for _, fn in legs:
            fn(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        raw_fed(20)
        steps = max(int(a.window * 20 / (time.perf_counter() - t0)), 20)          # each leg of each round lasts about --window
        rates = {k: [] for k, _ in legs}
        for _ in range(a.rounds):              # alternate the legs in one run
            for key, fn in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(steps)
                torch.cuda.synchronize()
                rates[key].append(round(a.bs * steps / (time.perf_counter() - t0), 1))
        res['detect'] = dict(target_size=dec.target_size, steps_per_leg=steps, images_per_s=rates)
        producer.shutdown()

    # the host baseline
    try:
        from PIL import Image
    except ImportError:
        res['pillow_ms_per_image'] = None
    else:
        def pil(b):
            return np.asarray(Image.open(io.BytesIO(b)).convert('RGB'))
        res['pillow_ms_per_image'] = {}
        for th in (1, 16):
            pool = ThreadPoolExecutor(th)
            many = data * 4
            res['pillow_ms_per_image'][str(th)] = wall_s(lambda: list(pool.map(pil, many)), a.window) * 1e3 / len(many)
            pool.shutdown()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
