"""The tracker behind the detector: Tracker.update takes what PPYOLO.forward_padded returns, where it lies, and BoxDrawer takes what
the tracker returns.  PPYOLO_r18vd with the synthetic weights at input side 320, three frames of one synthetic image shifted along
W; the tracker's result equals tests/track_ref.py on the model's own rows, byte for byte."""
import numpy as np
import pytest
import torch

import draw_ref
import track_ref as R

pytestmark = pytest.mark.gpu


def test_tracker_takes_forward_padded_and_the_drawer_takes_the_tracks():
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from ppyolo_hip import synth
    from ppyolo_hip.draw import BoxDrawer
    from ppyolo_hip.track import Tracker
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = 320
    model, _ = build_model(cfg, 0, 'cuda')
    x0 = synth.synth_images(1, 320).cuda()
    im_size = synth.synth_im_size(1).cuda()
    xs = [torch.roll(x0, shifts=4 * f, dims=3).contiguous() for f in range(3)]
    # the synthetic weights score low: the levels are set from the first frame's own scores, so that rows open tracks
    dets, count, _ = model.forward_padded(xs[0], im_size)
    n0 = int(count[0])
    assert n0 > 0
    scores = np.sort(dets[0, :n0, 1].cpu().numpy())
    high = float(scores[len(scores) // 2])
    kw = dict(max_tracks=64, high_thresh=high, new_thresh=high, low_thresh=float(scores[0]))
    tracker = Tracker(1, 'cuda', **kw)
    frames, got = [], []
    for x in xs:
        dets, count, _ = model.forward_padded(x, im_size)
        rows = tracker.update(dets, count)                  # the executor's own buffers, read in stream order
        frames.append((dets.cpu().numpy().copy(), count.cpu().numpy().copy()))
        got.append(tuple(t.cpu().numpy() for t in rows) + (tracker.state(),))
    want, refs = R.run(frames, **kw)
    for g, w in zip(got, want):
        for a, b in zip(g, w[:6]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert refs[0].issued > 0 and int(got[0][1][0]) > 0
    # the float64 run of the restatement makes the same matches on these rows
    for a, b in zip(want, R.run(frames, dtype=np.float64, **kw)[0]):
        assert a[7] == b[7] and np.array_equal(a[2], b[2])
    # the rows are forward_padded's format: the drawer takes them
    names = ['c%d' % i for i in range(80)]
    image = torch.full((int(im_size[0, 0]), int(im_size[0, 1]), 3), 128, dtype=torch.uint8, device='cuda')
    BoxDrawer(names, 'cuda')([image], rows[0], rows[1])
    ref = draw_ref.paint(np.full(tuple(image.shape), 128, np.uint8), got[-1][0][0], int(got[-1][1][0]), 0.0, names, draw_ref.colors_for(80))
    assert np.array_equal(image.cpu().numpy(), ref)
