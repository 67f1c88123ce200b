"""Timings of the draw launch (ppyolo_hip/draw.py BoxDrawer, csrc/draw.hip) on the decoded pixels of the two COCO-sized
fixtures of tests/golden/g20_jpeg.npz (500x375 and 640x418) replicated to a batch, in ONE process with the legs alternating:

  (a) draw, model    the draw launch with the R50vd-608 model's own detections of these images at draw_thresh 0.15 (synthetic
                     weights), replayed from a captured graph;
  (b) draw, worst    the draw launch with 100 rows per image, all drawn, boxes placed uniformly, replayed from a captured graph;
  (c) encoder        JpegEncoder's two device stages (1 + 8 launches) on the same pixels, replayed from captured graphs;
  (d) step           the one-lane detection step of the same run: Decode.detect_raw on the same pixels, R50vd-608;
  (e) annotate       Decode.annotate_files end to end on the files, host clock, beside Decode.detect_files.

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; the spread
(min .. max) is printed beside it.  The condition: (b) takes no longer than (c), the stage it feeds, in the same run -- the
draw touches only covered pixels, the encoder reads every pixel.

    python tools/draw_bench.py [--out profiles/draw_bench.txt] [--bs 8] [--seconds 1.0] [--rounds 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from jpeg_encode_bench import alternate, graph_of  # noqa: E402
from ppyolo_hip import _lib, ops  # noqa: E402
from ppyolo_hip.jpeg import JpegDecoder, JpegEncoder  # noqa: E402

COCO_NAMES = ['person', 'bicycle', 'car', 'motorbike', 'aeroplane', 'bus', 'train', 'truck', 'boat', 'traffic light', 'fire hydrant',
              'stop sign', 'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse', 'sheep', 'cow', 'elephant', 'bear', 'zebra', 'giraffe',
              'backpack', 'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis', 'snowboard', 'sports ball', 'kite', 'baseball bat',
              'baseball glove', 'skateboard', 'surfboard', 'tennis racket', 'bottle', 'wine glass', 'cup', 'fork', 'knife', 'spoon', 'bowl',
              'banana', 'apple', 'sandwich', 'orange', 'broccoli', 'carrot', 'hot dog', 'pizza', 'donut', 'cake', 'chair', 'sofa',
              'pottedplant', 'bed', 'diningtable', 'toilet', 'tvmonitor', 'laptop', 'mouse', 'remote', 'keyboard', 'cell phone', 'microwave',
              'oven', 'toaster', 'sink', 'refrigerator', 'book', 'clock', 'vase', 'scissors', 'teddy bear', 'hair drier', 'toothbrush']


def drawn_rows(dets, count, thresh, num_classes):
    d, c = dets.cpu().numpy(), count.cpu().numpy()
    n = 0
    for i in range(len(d)):
        r = d[i, :max(min(int(c[i]), d.shape[1]), 0)]
        ok = np.isfinite(r).all(axis=1) & (r[:, 1] >= np.float32(thresh)) & (r[:, 0] >= 0) & (r[:, 0] < num_classes) & (r[:, 1] >= 0) & (r[:, 1] <= 1)
        n += int(ok.sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'draw_bench.txt'))
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('draw_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    two_files = [g['jpg_' + str(n)].tobytes() for n in g['names'] if str(n).startswith('coco_')]
    files = [two_files[i % len(two_files)] for i in range(a.bs)]
    two = JpegDecoder().decode(two_files)
    pixels = [two[i % len(two)].clone() for i in range(a.bs)]
    say('%d images (%s); %s; windows >= %.1f s, %d rounds, legs alternating' % (
        a.bs, ', '.join('%dx%d' % (t.shape[1], t.shape[0]) for t in two), torch.cuda.get_device_name(0), a.seconds, a.rounds))

    from conftest import build_model
    from config import PPYOLO_2x_Config
    from model.decode_np import Decode
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg, 0, 'cuda')
    dec = Decode(model, COCO_NAMES, True, cfg, for_test=True)
    thresh = 0.15
    pimage, im_size = dec._preprocessor()(pixels)
    d_model, c_model, _ = model.forward_padded(pimage, im_size)
    d_model, c_model = d_model.clone(), c_model.clone()
    K = d_model.shape[1]

    rng = np.random.RandomState(0)
    worst = np.zeros((a.bs, 100, 6), np.float32)
    for i, t in enumerate(pixels):
        h, w = t.shape[:2]
        x0, y0 = rng.uniform(0, w - 8, 100), rng.uniform(0, h - 8, 100)
        worst[i, :, 0] = rng.randint(0, 80, 100)
        worst[i, :, 1] = rng.uniform(0.15, 1.0, 100)
        worst[i, :, 2], worst[i, :, 3] = x0, y0
        worst[i, :, 4], worst[i, :, 5] = x0 + rng.uniform(8, w, 100) * (1 - x0 / w), y0 + rng.uniform(8, h, 100) * (1 - y0 / h)
    d_worst = torch.from_numpy(worst).cuda()
    c_worst = torch.full((a.bs,), 100, dtype=torch.int32, device='cuda')

    drawer = dec.drawer()
    canvas = [t.clone() for t in pixels]               # the draw legs paint these; the encoder and the step read `pixels`
    drawer(canvas, d_worst, c_worst, thresh)           # uploads the tables
    colors, names, name_len, font = drawer._upload()
    descs = (_lib.DrawImage * a.bs)()
    for d, t in zip(descs, canvas):
        d.base, d.pitch, d.h, d.w = t.data_ptr(), t.stride(0), t.shape[0], t.shape[1]
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()

    def draw(dets, count):
        return lambda: ops.draw_detections(descs, table, dets, count, thresh, colors, names, name_len, drawer._h_name_len, font)

    n_model, n_worst = drawn_rows(d_model, c_model, thresh, 80), drawn_rows(d_worst, c_worst, thresh, 80)
    say('rows per image K = %d (model), 100 (worst case); draw_thresh %.2f' % (K, thresh))

    enc = JpegEncoder()
    eb = enc.coefficients(pixels)
    dev_out, lengths = enc.scan_device(eb)
    torch.cuda.synchronize()
    L = _lib.lib()
    ws = torch.empty(eb.sizes.ws_bytes, dtype=torch.uint8, device='cuda')

    def stage1():
        _lib.check(L.ppy_jpeg_enc_coefficients(eb.n, eb.descs, eb.table.data_ptr(), eb.coef.data_ptr(), eb.sizes.coef_bytes,
                                               torch.cuda.current_stream().cuda_stream), 'ppy_jpeg_enc_coefficients')

    def stage2():
        _lib.check(L.ppy_jpeg_enc_scan_device(eb.n, eb.descs, eb.table.data_ptr(), eb.coef.data_ptr(), eb.sizes.coef_bytes, dev_out.data_ptr(),
                                              eb.sizes.out_bytes, lengths.data_ptr(), ws.data_ptr(), eb.sizes.ws_bytes,
                                              torch.cuda.current_stream().cuda_stream), 'ppy_jpeg_enc_scan_device')

    legs = dict(draw_model=graph_of(draw(d_model, c_model)), draw_worst=graph_of(draw(d_worst, c_worst)), stage1=graph_of(stage1),
                stage2=graph_of(stage2), step=lambda: dec.detect_raw(pixels), annotate=lambda: dec.annotate_files(files, thresh),
                detect_files=lambda: dec.detect_files(files))
    r = alternate(legs, a.seconds, a.rounds)
    names_ = dict(draw_model='(a) draw, model\'s detections: %d rows drawn' % n_model, draw_worst='(b) draw, synthetic worst case: %d rows drawn' % n_worst,
                  stage1='(c) encoder stage 1, 1 launch', stage2='(c) encoder stage 2, 8 launches',
                  step='(d) one-lane detection step, R50vd-608 bs %d' % a.bs, annotate='(e) annotate_files, end to end',
                  detect_files='    detect_files, end to end')
    say()
    for k in legs:
        say('%-52s %9.3f ms per batch   (%.3f .. %.3f)' % (names_[k], r[k][0] * 1e3, r[k][1] * 1e3, r[k][2] * 1e3))
    both = r['stage1'][0] + r['stage2'][0]
    say()
    say('(c) both encoder stages %.3f ms per batch' % (both * 1e3))
    say('condition: (b) %.3f ms no longer than (c) %.3f ms in this run -> %s (%.2fx the encoder stages; %.3fx the detection step)' % (
        r['draw_worst'][0] * 1e3, both * 1e3, 'MET' if r['draw_worst'][0] <= both else 'MISSED', r['draw_worst'][0] / both,
        r['draw_worst'][0] / r['step'][0]))
    say('annotate_files - detect_files = %.3f ms per batch: the draw launch, both encoder stages, the read-back and the headers' % (
        (r['annotate'][0] - r['detect_files'][0]) * 1e3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
