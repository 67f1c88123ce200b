"""TiledDetector (ppyolo_hip/tiles.py) and Decode.detect_tiled / detect_tiled_files on r18vd at target size 64 with the synthetic
weights, on the two COCO-sized JPEG fixtures: the output equals, bit for bit, the numpy restatement tests/tile_merge_ref.py
applied to the rows that forward_padded gives for the same chunks built by hand through the public API."""
import numpy as np
import pytest
import torch

import tile_merge_ref as R

pytestmark = pytest.mark.gpu

BATCH = 8


@pytest.fixture(scope='module')
def detector():
    import jpeg_enc_cases as C
    import jpeg_fixtures as F
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    from ppyolo_hip.jpeg import JpegDecoder
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = 64
    model, _ = build_model(cfg, 0, 'cuda')
    dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
    files = [F.data(c[0]) for c in C.COCO]
    return dec, model, cfg, files, JpegDecoder().decode(files)


def rows_by_hand(model, cfg, images, views):
    """The rows of the views, chunk by chunk as TiledDetector runs them, but built through the public API alone: every view a
    contiguous copy, Preprocessor, forward_padded.  views: [(image, ox, oy, vw, vh)].  Returns numpy (dets [V, K, 6], count [V],
    table [V, 3]) with V a multiple of BATCH, the tail filled with view 0 marked -1."""
    from ppyolo_hip.preprocess import Preprocessor
    pre = Preprocessor(cfg, 64)
    padded = list(views) + [views[0]] * (-len(views) % BATCH)
    table = np.array([(i if j < len(views) else -1, ox, oy) for j, (i, ox, oy, vw, vh) in enumerate(padded)], dtype=np.int32)
    dets, count = [], []
    for lo in range(0, len(padded), BATCH):
        chunk = [images[i][oy:oy + vh, ox:ox + vw].contiguous() for i, ox, oy, vw, vh in padded[lo:lo + BATCH]]
        x, im_size = pre(chunk)
        assert im_size.cpu().tolist() == [[float(v[4]), float(v[3])] for v in padded[lo:lo + BATCH]]
        d, c, _ = model.forward_padded(x, im_size)
        dets.append(d.cpu().numpy().copy())
        count.append(c.cpu().numpy().copy())
    return np.concatenate(dets), np.concatenate(count), table


def thresholds_from_rows(dets, count, table, n):
    """(score_thresh, thresh) for 'ios' at which the batch selects at least one row and the scan suppresses at least one: the
    configuration's own (0.01, 0.5) if they do, else taken from the rows -- the median score, and half the largest metric
    between two admitted rows of an image (the later row of that pair, or an earlier casualty, is then suppressed)."""
    def stats(st, th):
        out = []
        R.merge_views(dets, count, table, n, 'ios', th, st, False, 100, stats=out)
        return sum(s['selected'] for s in out), sum(s['suppressed'] for s in out)
    st, th = 0.01, 0.5
    if stats(st, th)[0] == 0:
        live = np.concatenate([dets[v, :min(count[v], dets.shape[1]), 1] for v in range(len(count)) if table[v, 0] >= 0])
        st = float(np.median(live))
    if stats(st, th)[1] == 0:
        best = 0.0
        for i in range(n):
            src, boxes = R.merge_image(dets, count, table, i, 'ios', 1e30, st, True)      # every admitted row, translated, in order
            for j in range(1, len(src)):
                m = R.ios(boxes[j], boxes[:j])
                best = max(best, float(np.nanmax(np.where(np.isfinite(m), m, 0))))
        th = best / 2
    return st, th


def test_single_tile_image_is_the_models_own_rows_reordered(detector):
    from ppyolo_hip.preprocess import Preprocessor
    from ppyolo_hip.tiles import TiledDetector
    dec, model, cfg, files, images = detector
    # exactly 64 x 64: the first of eight candidates on which the model reports a row (seven windows read in place out of the
    # decoder's output, and the whole image subsampled)
    cands = [images[i][oy:oy + 64, ox:ox + 64] for i, ox, oy in ((0, 200, 100), (0, 0, 0), (0, 400, 300), (1, 100, 50), (1, 300, 200),
                                                                  (1, 500, 300), (1, 0, 354))]
    cands.append(images[0][::5, ::7][:64, :64].contiguous())
    assert all(tuple(t.shape) == (64, 64, 3) for t in cands)
    x, im_size = Preprocessor(cfg, 64)(cands)
    probe = model.forward_padded(x, im_size)[1].cpu().tolist()
    print('rows of the candidates', probe)
    assert max(probe) >= 1
    img = cands[[p >= 1 for p in probe].index(True)]
    x, im_size = Preprocessor(cfg, 64)([img] * BATCH)
    d, c, _ = model.forward_padded(x, im_size)
    d, c = d.cpu().numpy().copy(), c.cpu().numpy().copy()
    table = np.array([(0, 0, 0)] + [(-1, 0, 0)] * (BATCH - 1), dtype=np.int32)
    st = 0.01 if (d[0, :c[0], 1] >= 0.01).any() else float(np.median(d[0, :max(c[0], 1), 1]))
    tiled = TiledDetector(model, cfg, 64, full_view=False, metric='iou', thresh=1.0, score_thresh=st, batch=BATCH)
    got = [t.cpu().numpy() for t in tiled([img])]
    assert tiled.views == [(0, 0, 0, 64, 64)]
    want = R.merge_views(d, c, table, 1, 'iou', 1.0, st, False, cfg.nms_cfg['keep_top_k'])
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    k = int(got[1][0])
    assert k >= 1 and (got[2][0, :k, 0] == 0).all()
    rows = got[2][0, :k, 1]
    assert len(set(rows.tolist())) == k and (got[0][0, :k] == d[0, rows]).all()          # the model's rows, untouched (offset 0)
    assert (np.diff(got[0][0, :k, 1]) <= 0).all()


def test_tiled_output_equals_the_restatement_on_hand_built_chunks(detector):
    from ppyolo_hip import tiles
    from ppyolo_hip.tiles import TiledDetector
    dec, model, cfg, files, images = detector
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
    views = [(i, ox, oy, vw, vh) for i, (h, w) in enumerate(sizes) for ox, oy, vw, vh in tiles.plan_views(h, w, 192, 0.2, True)]
    assert [sum(1 for v in views if v[0] == i) for i in (0, 1)] == [13, 13]
    d, c, table = rows_by_hand(model, cfg, images, views)
    assert d.shape[0] == 32 and (table[26:, 0] == -1).all()
    st, th = thresholds_from_rows(d, c, table, 2)
    print('score_thresh %r thresh %r rows %s' % (st, th, c.tolist()))
    stats = []
    want = R.merge_views(d, c, table, 2, 'ios', th, st, False, 100, stats=stats)
    print(stats)
    assert sum(s['selected'] for s in stats) >= 1 and sum(s['suppressed'] for s in stats) >= 1
    tiled = TiledDetector(model, cfg, 64, tile=192, overlap=0.2, metric='ios', thresh=th, score_thresh=st, batch=BATCH)
    got = [t.cpu().numpy() for t in tiled(images)]
    assert tiled.views == views
    for g, w, name in zip(got, want, ('dets', 'count', 'src')):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name
    again = [t.cpu().numpy() for t in tiled(images)]                    # the same detector, its buffers reused
    for g, w in zip(again, want):
        assert g.tobytes() == w.tobytes()
    # the other mode, class-agnostic IoU, through the same rows
    tiled2 = TiledDetector(model, cfg, 64, tile=192, metric='iou', thresh=th, score_thresh=st, class_agnostic=True, keep_top_k=7, batch=BATCH)
    got2 = [t.cpu().numpy() for t in tiled2(images)]
    for g, w in zip(got2, R.merge_views(d, c, table, 2, 'iou', th, st, True, 7)):
        assert g.tobytes() == w.tobytes()


def test_result_feeds_the_drawer_and_the_cropper_unchanged(detector):
    import pil_crop_ref as cref
    from ppyolo_hip.crops import DetectionCropper
    from ppyolo_hip.draw import BoxDrawer
    from ppyolo_hip.tiles import TiledDetector
    dec, model, cfg, files, images = detector
    tiled = TiledDetector(model, cfg, 64, tile=192, score_thresh=0.0, batch=BATCH)
    dets, count, src = tiled(images)
    assert dets.dtype == torch.float32 and tuple(dets.shape) == (2, 100, 6) and count.dtype == torch.int32 and tuple(count.shape) == (2,)
    d, c = dets.cpu().numpy(), count.cpu().numpy()
    assert c.sum() >= 1
    thresh = float(np.median(d[0, :max(c[0], 1), 1]))
    # the cropper: its own selection rule on these rows
    crops, csrc, total = DetectionCropper((32, 24))(images, dets, count, thresh=thresh)
    want_src, _ = cref.select_rows(d, c, [tuple(t.shape[:2]) for t in images], thresh, 0.0, None)
    t = int(total.cpu()[0])
    assert t == len(want_src) and csrc[:t].cpu().tolist() == [list(s) for s in want_src]
    # the drawer: the same pixels as from a fresh copy of the rows
    drawer = BoxDrawer(['c%d' % i for i in range(80)])
    a = [im.clone() for im in images]
    b = [im.clone() for im in images]
    drawer(a, dets, count, thresh)
    drawer(b, torch.from_numpy(d.copy()).cuda(), torch.from_numpy(c.copy()).cuda(), thresh)
    for x, y, im in zip(a, b, images):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, im) for x, im in zip(a, images)) or not ((d[:, :, 1] >= thresh) & (np.arange(100)[None] < c[:, None])).any()


def test_detect_tiled_files_equals_detect_tiled_of_the_decoded_images(detector):
    dec, model, cfg, files, images = detector
    kw = dict(tile=192, score_thresh=0.0, keep_top_k=50)
    a = dec.detect_tiled_files(files, **kw)
    first = dec._tiled
    b = dec.detect_tiled(images, **kw)
    assert dec._tiled is first                                          # kept, keyed by its settings
    assert len(a) == len(b) == 2
    for (ab, as_, ac), (bb, bs, bc) in zip(a, b):
        assert np.array_equal(ab, bb) and np.array_equal(as_, bs) and np.array_equal(ac, bc)
    assert sum(len(s) for _, s, _ in a) >= 1
    dets, count, _ = first(images)
    d, c = dets.cpu().numpy(), count.cpu().tolist()
    for i, (bx, sc, cl) in enumerate(a):
        if c[i] == 0:                                                   # _split's "no detection" form
            assert len(bx) == len(sc) == len(cl) == 0
            continue
        assert np.array_equal(bx, d[i, :c[i], 2:]) and np.array_equal(sc, d[i, :c[i], 1]) and np.array_equal(cl, d[i, :c[i], 0].astype(np.int32))
    dec.detect_tiled(images, tile=192, score_thresh=0.0, keep_top_k=51)
    assert dec._tiled is not first
