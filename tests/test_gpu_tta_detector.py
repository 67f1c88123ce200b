"""TtaDetector (ppyolo_hip/tta.py) and Decode.detect_tta / detect_tta_files on r18vd at the input sides (64, 96) with mirrored
views and the synthetic weights, on the two COCO-sized JPEG fixtures: the output equals, bit for bit, the numpy restatement
tests/fuse_views_ref.py applied to the rows that forward_padded gives for the same chunks built by hand through the public API
(Preprocessor, torch.flip, forward_padded)."""
import numpy as np
import pytest
import torch

import fuse_views_ref as R

pytestmark = pytest.mark.gpu

BATCH = 8
SCALES = (64, 96)


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


def rows_by_hand(model, cfg, images, scales, hflip):
    """The rows of the views, chunk by chunk as TtaDetector runs them, but built through the public API alone.  Returns numpy
    (dets [V, K, 6], count [V], table [V, 4], views [(image or -1, side, flipped)])."""
    from ppyolo_hip.preprocess import Preprocessor
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
    dets, count, table, views = [], [], [], []
    for S in scales:
        x, im_size = Preprocessor(cfg, S)(images)
        assert im_size.cpu().tolist() == [[float(h), float(w)] for h, w in sizes]
        xs, rows = [], []
        for i in range(len(images)):
            for f in ((0, 1) if hflip else (0,)):
                xs.append(torch.flip(x[i], dims=[2]) if f else x[i])
                rows.append((i, 0, 0, sizes[i][1] if f else 0, f))
        pad = -len(xs) % BATCH
        xs += [xs[0]] * pad
        rows += [(-1, 0, 0, 0, 0)] * pad
        for lo in range(0, len(xs), BATCH):
            sz = torch.tensor([sizes[max(r[0], 0)] for r in rows[lo:lo + BATCH]], dtype=torch.float32).cuda()
            d, c, _ = model.forward_padded(torch.stack(xs[lo:lo + BATCH]).contiguous(), sz)
            dets.append(d.cpu().numpy().copy())
            count.append(c.cpu().numpy().copy())
        table += [r[:4] for r in rows]
        views += [(r[0], S, bool(r[4])) for r in rows]
    return np.concatenate(dets), np.concatenate(count), np.array(table, dtype=np.int32), views


def thresholds_from_rows(dets, count, table, weight, n):
    """(score_thresh, thresh) at which the batch forms at least one cluster of several rows: the defaults (0.01, 0.55) if they do,
    else taken from the rows -- the median score, and half the largest IoU between two admitted rows of one image and class."""
    def most(st, th):
        out = []
        R.fuse_views(dets, count, table, weight, n, th, st, 100, stats=out)
        return max(s['max_members'] for s in out)
    st, th = 0.01, 0.55
    live = np.concatenate([dets[v, :min(count[v], dets.shape[1]), 1] for v in range(len(count)) if table[v, 0] >= 0])
    if not (live >= st).any():
        st = float(np.median(live))
    if most(st, th) < 2:
        best = 0.0
        for i in range(n):
            adm = R.admitted_rows(dets, count, table, i, st)
            for j in range(1, len(adm)):
                prev = [a for a in adm[:j] if int(dets[a[0], a[1], 0]) == int(dets[adm[j][0], adm[j][1], 0])]
                if prev:
                    m = R.iou(adm[j][2], np.stack([a[2] for a in prev]))
                    best = max(best, float(np.nanmax(np.where(np.isfinite(m), m, 0))))
        th = best / 2
    return st, th


def test_tta_output_equals_the_restatement_on_hand_built_chunks(detector):
    """Both fixtures, sides 64 and 96, mirrored: 8 views in two chunks of 8, four of each chunk padding.  With the synthetic weights
    the second fixture gives the overlapping pair at the defaults (score 0.01, IoU 0.55): its four views report 4, 5, 18 and 21
    rows, 48 admitted, 45 clusters, one of them of two rows; the first fixture reports no row.  Were there no cluster of several
    rows the thresholds are taken from the rows, and without any overlapping pair this test fails, it does not skip."""
    from ppyolo_hip.tta import TtaDetector
    dec, model, cfg, files, images = detector
    d, c, table, views = rows_by_hand(model, cfg, images, SCALES, True)
    assert d.shape[0] == 16 and table[:, 0].tolist() == [0, 0, 1, 1, -1, -1, -1, -1] * 2
    assert table[:4, 3].tolist() == [0, images[0].shape[1], 0, images[1].shape[1]]
    weight = np.ones((16,), dtype=np.float32)
    st, th = thresholds_from_rows(d, c, table, weight, 2)
    stats = []
    want = R.fuse_views(d, c, table, weight, 2, th, st, 100, stats=stats)
    print('score_thresh %r thresh %r rows %s' % (st, th, c.tolist()))
    print(stats)
    assert max(s['max_members'] for s in stats) >= 2
    tta = TtaDetector(model, cfg, scales=SCALES, hflip=True, thresh=th, score_thresh=st, batch=BATCH)
    got = [t.cpu().numpy() for t in tta(images)]
    assert tta.views == views
    for g, w, name in zip(got, want, ('dets', 'count', 'src', 'members')):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name
    again = [t.cpu().numpy() for t in tta(images)]                      # the same detector, its buffers reused
    for g, w in zip(again, want):
        assert g.tobytes() == w.tobytes()
    # per-view weights and another cut, through the same rows
    wts = [[1.0, 0.5], [2.0, 1.5]]
    weight2 = np.array([wts[SCALES.index(S)][int(f)] for _, S, f in views], dtype=np.float32)
    tta2 = TtaDetector(model, cfg, scales=SCALES, hflip=True, weights=wts, thresh=th, score_thresh=st, keep_top_k=7, batch=BATCH)
    got2 = [t.cpu().numpy() for t in tta2(images)]
    for g, w in zip(got2, R.fuse_views(d, c, table, weight2, 2, th, st, 7)):
        assert g.tobytes() == w.tobytes()


def test_one_plain_scale_at_thresh_one_is_the_models_own_rows(detector):
    from ppyolo_hip.tta import TtaDetector
    dec, model, cfg, files, images = detector
    d, c, table, views = rows_by_hand(model, cfg, images, (64,), False)
    assert table[:, 0].tolist() == [0, 1] + [-1] * 6 and c[:2].sum() >= 1
    live = np.concatenate([d[v, :c[v], 1] for v in (0, 1)])
    st = 0.01 if (live >= 0.01).any() else float(np.median(live))
    tta = TtaDetector(model, cfg, scales=(64,), hflip=False, thresh=1.0, score_thresh=st, batch=BATCH)
    dets, count, src, members = [t.cpu().numpy() for t in tta(images)]
    assert tta.views == views and count.sum() >= 1
    for i in range(2):
        k = int(count[i])
        assert k == len(R.admitted_rows(d, c, table, i, st)) and (members[i, :k] == 1).all() and (members[i, k:] == -1).all()
        assert (src[i, :k, 0] == i).all() and len(set(src[i, :k, 1].tolist())) == k
        own = d[i, src[i, :k, 1]].copy()
        own[:, 2:6] = own[:, 2:6] + np.float32(0)      # the contract adds the view's origin, here 0: a -0.0 of the decode becomes +0.0
        assert dets[i, :k].tobytes() == own.tobytes()                          # class, score and box of the model's rows, bit for bit
        assert (np.diff(dets[i, :k, 1]) <= 0).all()


def test_result_feeds_the_drawer_and_the_cropper_unchanged(detector):
    import pil_crop_ref as cref
    from ppyolo_hip.crops import DetectionCropper
    from ppyolo_hip.draw import BoxDrawer
    from ppyolo_hip.tta import TtaDetector
    dec, model, cfg, files, images = detector
    tta = TtaDetector(model, cfg, scales=SCALES, score_thresh=1e-6, batch=BATCH)
    dets, count, src, members = tta(images)
    assert dets.dtype == torch.float32 and tuple(dets.shape) == (2, 100, 6) and count.dtype == torch.int32 and tuple(count.shape) == (2,)
    d, c = dets.cpu().numpy(), count.cpu().numpy()
    assert c.sum() >= 1
    thresh = float(np.median(d[0, :max(c[0], 1), 1]))
    crops, csrc, total = DetectionCropper((32, 24))(images, dets, count, thresh=thresh)
    want_src, _ = cref.select_rows(d, c, [tuple(t.shape[:2]) for t in images], thresh, 0.0, None)
    t = int(total.cpu()[0])
    assert t == len(want_src) and csrc[:t].cpu().tolist() == [list(s) for s in want_src]
    drawer = BoxDrawer(['c%d' % i for i in range(80)])
    a = [im.clone() for im in images]
    b = [im.clone() for im in images]
    drawer(a, dets, count, thresh)
    drawer(b, torch.from_numpy(d.copy()).cuda(), torch.from_numpy(c.copy()).cuda(), thresh)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, im) for x, im in zip(a, images)) or not ((d[:, :, 1] >= thresh) & (np.arange(100)[None] < c[:, None])).any()


def test_detect_tta_files_equals_detect_tta_of_the_decoded_images(detector):
    dec, model, cfg, files, images = detector
    kw = dict(scales=SCALES, score_thresh=1e-6, keep_top_k=50)
    a = dec.detect_tta_files(files, **kw)
    first = dec._tta
    b = dec.detect_tta(images, **kw)
    assert dec._tta is first                                            # kept, keyed by its settings
    assert len(a) == len(b) == 2
    for (ab, as_, ac), (bb, bs, bc) in zip(a, b):
        assert np.array_equal(ab, bb) and np.array_equal(as_, bs) and np.array_equal(ac, bc)
    assert sum(len(s) for _, s, _ in a) >= 1
    dets, count, _, _ = first(images)
    d, c = dets.cpu().numpy(), count.cpu().tolist()
    for i, (bx, sc, cl) in enumerate(a):
        if c[i] == 0:                                                   # _split's "no detection" form
            assert len(bx) == len(sc) == len(cl) == 0
            continue
        assert np.array_equal(bx, d[i, :c[i], 2:]) and np.array_equal(sc, d[i, :c[i], 1]) and np.array_equal(cl, d[i, :c[i], 0].astype(np.int32))
    dec.detect_tta(images, scales=SCALES, score_thresh=1e-6, keep_top_k=51)
    assert dec._tta is not first
    assert dec.detect_tta(images, score_thresh=1e-6) is not None and dec._tta.scales == (64,)      # default: the target size
