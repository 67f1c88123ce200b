"""PngDecoder on the device (csrc/png.hip, ppyolo_hip/png.py) against the numpy restatement (tests/png_ref.py, itself held to
Pillow by tests/test_png_host.py), tests/golden/g26_png.npz and the installed Pillow; ImageDecoder through the file-fed entry
points.  Array equality everywhere: there is no tolerance."""
import ctypes
import io
import warnings
import zlib

import numpy as np
import pytest
import torch

import png_cases as C
import png_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dec():
    from ppyolo_hip.png import PngDecoder
    return PngDecoder()


def _differences(got, want, name):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (name, got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    y, x, c = bad[0]
    return '%s: %d of %d bytes differ, first at (y %d, x %d, c %d): got %d, want %d' % (name, len(bad), want.size, y, x, c, got[y, x, c], want[y, x, c])


def check_batch(dec, names):
    cases = C.all_cases()
    outs = dec.decode([cases[n] for n in names])
    assert len(outs) == len(names) and all(t.is_cuda and t.dtype == torch.uint8 for t in outs)
    wrong = [d for d in (_differences(t, C.want(n), n) for n, t in zip(names, outs)) if d]
    assert not wrong, '%d of %d files:\n%s' % (len(wrong), len(names), '\n'.join(wrong[:12]))


def test_edges_and_filter_arithmetic(dec):
    check_batch(dec, sorted(C.edges()))


def test_every_format_sub_byte_widths_and_palettes(dec):
    check_batch(dec, sorted(C.formats()))


def test_rows_in_flight_band_hand_over_and_staging_widths(dec):
    check_batch(dec, sorted(C.rows_and_widths()))


def test_adam7(dec):
    check_batch(dec, sorted(C.adam7()))


@pytest.mark.parametrize('name', ['edge_c2_d8_1x1_first4', 'rows_1025x3', 'rows_1030x40_rgba', 'adam7_c6_d16_37x23', 'sub_c0_d1_w9'])
def test_single_file_calls(dec, name):
    """A call of its own sizes the launch from this file alone (one wave for a 1x1 image, 1024 rows in flight for the tall one)."""
    assert _differences(dec.imdecode(C.all_cases()[name]), C.want(name), name) is None


def test_one_batch_mixes_everything_and_out_views_keep_their_guards(dec):
    names = sorted(C.all_cases())
    check_batch(dec, names)
    cases = C.all_cases()
    wants = [C.want(n) for n in names]
    wide = [torch.full((w.shape[0] + 2, w.shape[1] + 2 + k % 5, 3), 0xA5, dtype=torch.uint8, device='cuda') for k, w in enumerate(wants)]
    views = [b[1:1 + w.shape[0], 1 + k % 2:1 + k % 2 + w.shape[1]] for k, (b, w) in enumerate(zip(wide, wants))]
    got = dec.decode([cases[n] for n in names], out=views)
    assert all(a is b for a, b in zip(got, views))
    for k, (n, b, w) in enumerate(zip(names, wide, wants)):
        full = b.cpu().numpy()
        x0 = 1 + k % 2
        assert np.array_equal(full[1:1 + w.shape[0], x0:x0 + w.shape[1]], w), n
        full[1:1 + w.shape[0], x0:x0 + w.shape[1]] = 0xA5
        assert np.all(full == 0xA5), (n, 'bytes around the view were written')


def test_outputs_are_refused_by_name(dec):
    from ppyolo_hip._lib import PPYoloHipError
    data = C.all_cases()['fmt_c2_d8']                                               # 5 x 7
    ok = torch.empty((5, 7, 3), dtype=torch.uint8, device='cuda')
    for bad, word in ((torch.empty((5, 7, 3), dtype=torch.uint8), 'uint8 device tensor'), (torch.empty((7, 5, 3), dtype=torch.uint8, device='cuda'), r'\[5, 7, 3\]'),
                      (torch.empty((5, 7, 3), dtype=torch.float32, device='cuda'), 'uint8 device tensor'),
                      (torch.empty((5, 7, 4), dtype=torch.uint8, device='cuda')[:, :, :3], 'pixel stride 3'),
                      (torch.empty((5, 3, 7), dtype=torch.uint8, device='cuda').permute(0, 2, 1), 'pixel stride 3')):
        with pytest.raises(PPYoloHipError, match='output 0.*' + word):
            dec.decode([data], out=[bad])
    with pytest.raises(PPYoloHipError, match='2 output tensors for 1 images'):
        dec.decode([data], out=[ok, ok])
    assert dec.decode([data], out=[ok])[0] is ok and np.array_equal(ok.cpu().numpy(), C.want('fmt_c2_d8'))


def test_host_batches_own_their_staging_buffer():
    """tests/test_gpu_jpeg.py's test of the same name for PngDecoder: a third waiting batch is refused, a refused file gives its
    buffer back, the same batch may be reconstructed twice, a released or overtaken batch is stale."""
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.png import PngDecoder
    cases = C.all_cases()
    names = ['edge_c2_d8_1x1_first0', 'edge_c0_d8_2x2_first4', 'edge_c6_d16_1x9_first1', 'edge_c2_d8_9x1_first2', 'edge_tie3_wrap']

    def same(hb, name):
        return _differences(d.reconstruct(hb)[0], C.want(name), name) is None

    d = PngDecoder()
    a = d.host_decode([cases[names[0]]])
    b = d.host_decode([cases[names[1]]])
    with pytest.raises(PPYoloHipError, match='the host stage may run at most two batches ahead'):
        d.host_decode([cases[names[2]]])
    assert same(b, names[1])
    with pytest.raises(PPYoloHipError, match='item 0: corrupt PNG'):    # a refused file gives its buffer back
        d.host_decode([sorted(C.damaged().items())[0][1][0]])
    assert same(a, names[0])
    assert same(a, names[0])                                            # again, while it is still the buffer's batch
    c = d.host_decode([cases[names[2]]])
    d.release(c)
    e1 = d.host_decode([cases[names[3]]])
    e2 = d.host_decode([cases[names[4]]])
    assert all((h.slot, h.gen) not in ((e1.slot, e1.gen), (e2.slot, e2.gen)) for h in (a, b, c))
    for h in (a, b, c):
        with pytest.raises(PPYoloHipError, match='stale HostBatch'):
            d.reconstruct(h)
    assert same(e2, names[4]) and same(e1, names[3])


def test_a_corrupt_item_is_named(dec):
    from ppyolo_hip._lib import PPYoloHipError
    cases = C.all_cases()
    good = [cases['fmt_c2_d8'], cases['adam7_c2_d8_9x9'], cases['pal_16']]
    for name, (data, kind, word) in C.damaged().items():
        with pytest.raises(PPYoloHipError, match=r'^item 2: %s PNG: .*%s' % (kind, word)):
            dec.decode(good[:2] + [data] + good[2:])
    check_batch(dec, ['fmt_c2_d8', 'adam7_c2_d8_9x9', 'pal_16'])                    # the decoder is usable afterwards


def test_run_to_run_and_graph_replay(dec):
    from ppyolo_hip import _lib
    names = ['rows_1030x40_rgba', 'adam7_c6_d16_37x23', 'width_65', 'sub_c3_d2_w17', 'edge_two_all4', 'rows_129']
    cases = C.all_cases()
    first = [t.clone() for t in dec.decode([cases[n] for n in names])]
    for _ in range(3):
        assert all(torch.equal(a, b) for a, b in zip(first, dec.decode([cases[n] for n in names])))
    # the launches alone, as a C caller enqueues them: captured once, replayed into cleared outputs
    L = _lib.lib()
    hb = dec.host_decode([cases[n] for n in names])
    outs = [torch.zeros_like(t) for t in first]
    n = hb.n
    _lib.check(L.ppy_png_pack_table(n, hb.descs, (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs]),
                                    (ctypes.c_longlong * n)(*[t.stride(0) for t in outs]), hb.stage.data_ptr(), hb.table_bytes))
    blob = hb.stage[:hb.total_bytes].cuda()
    dec.release(hb)
    ws_bytes = L.ppy_png_workspace_bytes(n, hb.descs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')

    def launch():
        _lib.check(L.ppy_png_reconstruct_u8(n, hb.descs, blob.data_ptr(), blob.data_ptr() + hb.table_bytes, hb.total_bytes - hb.table_bytes,
                                            ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream), 'ppy_png_reconstruct_u8')
    launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, outs))


def _smooth(h, w, seed):
    """An image with structure, so that libpng's adaptive choice uses several filter types."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 37.0 + y / 53.0), 128 + 90 * np.cos(x / 23.0), (x * 255 // w + y * 3) % 256], -1)
    img = np.clip(base + rng.randint(-6, 7, (h, w, 3)) * (x[..., None] > w // 3), 0, 255).astype(np.uint8)
    q = h // 4
    img[q:2 * q] = rng.randint(0, 256, (1, w, 3))                      # columns that repeat down the rows: Up
    img[2 * q:3 * q] = rng.randint(0, 256, (q, w, 3))                  # noise: None
    return img


def _pillow_png(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, 'PNG', **kw)
    return buf.getvalue()


def test_coco_sized_file_written_by_pillow_and_the_golden_set(dec):
    from PIL import Image
    rgb = _smooth(418, 640, 26)
    data = _pillow_png(rgb)
    raw = zlib.decompress(b''.join(b for t, b in png_ref.chunks(data) if t == b'IDAT'))
    filters = set(np.frombuffer(raw, np.uint8)[::1 + 3 * 640].tolist())
    assert len(filters) >= 3, filters                                               # adaptive: several filter types in one file
    assert _differences(dec.imdecode(data), np.ascontiguousarray(rgb[..., ::-1]), 'coco-sized') is None
    g = C.golden()
    names = [str(n) for n in g['names']]
    outs = dec.decode([g['png_' + n].tobytes() for n in names])
    for n, t in zip(names, outs):
        assert _differences(t, g['bgr_' + n], n) is None
        data = g['png_' + n].tobytes()
        if not C.is_grey16(data):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                installed = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[..., ::-1]
            assert np.array_equal(t.cpu().numpy(), installed), (n, 'installed Pillow')


# ---- the file-fed entry points with decoder=ImageDecoder() ------------------------------------------------------------------------
def _detector(size=320):
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = size
    model, _ = build_model(cfg, 0, 'cuda')
    return Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True), cfg


def _small_jpegs():
    import jpeg_fixtures as F
    return F, [n for n in F.names() if 'bgr_' + n in F.golden() and min(F.golden()['bgr_' + n].shape[:2]) >= 16][:2]


def test_detect_files_on_mixed_jpeg_and_png_paths(tmp_path):
    from ppyolo_hip.imagefile import ImageDecoder
    from ppyolo_hip.jpeg import JpegDecoder
    from ppyolo_hip.png import PngDecoder
    F, jpegs = _small_jpegs()
    pngs = [_pillow_png(_smooth(70, 90, 1)), C.all_cases()['adam7_c2_d8_37x23'], _pillow_png(_smooth(48, 33, 2)[..., 0])]
    files = [pngs[0], F.data(jpegs[0]), pngs[1], F.data(jpegs[1]), pngs[2]]
    paths = []
    for k, data in enumerate(files):
        p = tmp_path / ('image_%d.%s' % (k, 'png' if data[:4] == b'\x89PNG' else 'jpg'))
        p.write_bytes(data)
        paths.append(str(p))
    det, _ = _detector()
    got = det.detect_files(paths, decoder=ImageDecoder())
    j, p = JpegDecoder().decode([files[1], files[3]]), PngDecoder().decode([files[0], files[2], files[4]])
    want = det.detect_raw([p[0], j[0], p[1], j[1], p[2]])
    assert len(got) == len(want) == 5
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            assert a.shape == b.shape and np.array_equal(a, b), k
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError, match='item 0'):                              # without decoder=, a PNG behaves as before
        det.detect_files(paths[:1])


def test_from_files_on_png_twins_equals_the_device_source_batch():
    from config import PPYOLO_2x_Config
    from ppyolo_hip import augment as A
    from ppyolo_hip.imagefile import ImageDecoder
    F, names = _small_jpegs()

    def records(image_of):
        rng = np.random.RandomState(17)
        out = []
        for name in names:
            h, w = F.golden()['bgr_' + name].shape[:2]
            G = 2
            x1, y1 = rng.uniform(0, w - 8, G), rng.uniform(0, h - 8, G)
            box = np.stack([x1, y1, x1 + rng.uniform(4, 7, G), y1 + rng.uniform(4, 7, G)], 1).astype(np.float32)
            r = dict(h=h, w=w, gt_bbox=box, gt_class=rng.randint(0, 80, (G, 1)).astype(np.int32), gt_score=np.ones((G, 1), np.float32),
                     is_crowd=np.zeros((G, 1), np.int32))
            r.update(image_of(name))
            out.append(r)
        return out

    b50 = A.TrainBatchBuilder(PPYOLO_2x_Config())
    pixels = lambda n: torch.from_numpy(np.ascontiguousarray(F.golden()['bgr_' + n])).cuda()      # noqa: E731
    twin = lambda n: _pillow_png(np.ascontiguousarray(F.golden()['bgr_' + n][..., ::-1]))           # noqa: E731
    want = {k: v.clone() for k, v in b50(records(lambda n: dict(image=pixels(n))), 64, np.random.RandomState(17)).items()}
    got = b50.from_files(records(lambda n: dict(image=twin(n))), 64, np.random.RandomState(17), decoder=ImageDecoder())
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_annotate_files_runs_on_a_png_input():
    from ppyolo_hip.imagefile import ImageDecoder
    det, cfg = _detector()
    cfg.test_cfg['draw_thresh'] = 0.02
    data = _pillow_png(_smooth(120, 160, 3))
    files, results = det.annotate_files([data], decoder=ImageDecoder())
    plain = det.detect_files([data], decoder=ImageDecoder())
    assert len(files) == len(results) == 1 and files[0][:2] == b'\xff\xd8' and files[0][-2:] == b'\xff\xd9'
    for a, b in zip(results[0], plain[0]):
        assert a.shape == b.shape and np.array_equal(a, b)
