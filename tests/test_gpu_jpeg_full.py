"""JpegDecoder(accept=...) on the device: progressive files, sequential files in several scans and the further luma sampling
factors, against the libjpeg-turbo pixels of tests/golden/g22_jpeg_full.npz and against tests/jpeg_full_ref.py.  Array
equality everywhere; Pillow is not needed."""
import numpy as np
import pytest
import torch

import jpeg_fixtures as F20
import jpeg_full_fixtures as F
import jpeg_full_ref as FR
import jpeg_full_synth as FS
from test_gpu_jpeg_synth import device_reconstruct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dec():
    from ppyolo_hip.jpeg import JpegDecoder
    return JpegDecoder(accept='all')


def test_mixed_batch_of_new_and_baseline_files(dec):
    """Every new golden and every baseline fixture in ONE call (still two launches), and the progressive fixture the baseline
    goldens keep as a refusal."""
    new, old = F.names(), F20.names()
    outs = dec.decode([F.data(n) for n in new] + [F20.data(n) for n in old] + [F20.data('progressive_30x30')])
    assert len(outs) == len(new) + len(old) + 1
    for n, t in zip(new, outs):
        assert t.is_cuda and t.dtype == torch.uint8 and F.matches_golden(n, t.cpu().numpy()), n
    for n, t in zip(old, outs[len(new):]):
        assert F20.matches_golden(n, t.cpu().numpy()), n
    assert np.array_equal(outs[-1].cpu().numpy(), FR.decode(F20.data('progressive_30x30')))


SEAM_SIZES = [(1, 1), (2, 3), (9, 5), (23, 17), (70, 40)]               # (H, W): the sizes of the goldens


@pytest.mark.parametrize('luma', sorted(FS.NEW_LUMA))
def test_new_samplings_from_the_seam(luma):
    """Seeded coefficients (padding blocks included) through ppy_jpeg_pack_table / ppy_jpeg_reconstruct_u8: every size x the
    eight orientations in one batch, then the same images into row-strided views."""
    rng = np.random.default_rng(2210)
    hds = [FS.synth(rng, H, W, FS.NEW_LUMA[luma], orientation=o) for H, W in SEAM_SIZES for o in range(1, 9)]
    want = [FR.reconstruct(hd) for hd in hds]
    for t, w, hd in zip(device_reconstruct(hds), want, hds):
        assert tuple(t.shape) == w.shape and np.array_equal(t.cpu().numpy(), w), (luma, hd['H'], hd['W'], hd['orientation'])
    wide = [torch.full((w.shape[0], w.shape[1] + 1 + k % 4, 3), 0xA5, dtype=torch.uint8, device='cuda') for k, w in enumerate(want)]
    device_reconstruct(hds, out=[b[:, 1:1 + w.shape[1]] for b, w in zip(wide, want)])
    for b, w, hd in zip(wide, want, hds):
        got = b.cpu().numpy()
        assert np.array_equal(got[:, 1:1 + w.shape[1]], w), (luma, hd['H'], hd['W'], hd['orientation'])
        assert np.all(got[:, :1] == 0xA5) and np.all(got[:, 1 + w.shape[1]:] == 0xA5)


def test_each_option_lifts_its_own_refusal():
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.jpeg import JpegDecoder
    y440 = F.data('syn_440_single_1x1')
    prog = F.data('pil_p420_q35_7x9')
    only_prog = JpegDecoder(accept={'progressive'})
    assert only_prog.refusal(prog) is None and F.matches_golden('pil_p420_q35_7x9', only_prog.imdecode(prog).cpu().numpy())
    kind, reason = only_prog.refusal(y440)
    assert kind == 'unsupported' and 'sampling factors' in reason
    with pytest.raises(PPYoloHipError, match='unsupported JPEG: sampling factors'):
        only_prog.imdecode(y440)
    assert F.matches_golden('syn_440_single_1x1', JpegDecoder(accept='sampling').imdecode(y440).cpu().numpy())
    assert JpegDecoder().refusal(prog) == ('unsupported', 'progressive JPEG')
    assert JpegDecoder(accept=['multiscan', 'sampling']).refusal(prog) == ('unsupported', 'progressive JPEG')
    assert JpegDecoder(accept='all').refusal(F.data(F.incomplete()[0])) is None         # the header pass cannot see the script's end
    with pytest.raises(PPYoloHipError, match='incomplete progressive scan script'):
        JpegDecoder(accept='all').imdecode(F.data(F.incomplete()[0]))
    with pytest.raises(PPYoloHipError, match='accept must be'):
        JpegDecoder(accept='everything')


@pytest.mark.parametrize('accept', ['all', {'progressive'}, ['sampling'], 'multiscan'])
def test_device_entropy_mode_takes_baseline_only(accept):
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.jpeg import JpegDecoder
    with pytest.raises(PPYoloHipError, match='device entropy stage reads single-scan baseline files only'):
        JpegDecoder(entropy='device', accept=accept)
    assert JpegDecoder(entropy='device', accept='baseline').accept == 0


_PAIR = ['pil_p422_q75_dri1_37x53', 'syn_440_default_17x23']           # one progressive, one 4:4:0 (progressive as well)


def _records(image_of):
    rng = np.random.RandomState(17)
    out = []
    for name in _PAIR:
        h, w = F.golden()['bgr_' + name].shape[:2]
        G = 2
        x1, y1 = rng.uniform(0, w - 8, G), rng.uniform(0, h - 8, G)
        box = np.stack([x1, y1, x1 + rng.uniform(4, 7, G), y1 + rng.uniform(4, 7, G)], 1).astype(np.float32)
        r = dict(h=h, w=w, gt_bbox=box, gt_class=rng.randint(0, 80, (G, 1)).astype(np.int32), gt_score=np.ones((G, 1), np.float32),
                 is_crowd=np.zeros((G, 1), np.int32))
        r.update(image_of(name))
        out.append(r)
    return out


def test_from_files_equals_the_batch_from_device_sources(dec):
    from config import PPYOLO_2x_Config
    from ppyolo_hip import augment as A
    from ppyolo_hip._lib import PPYoloHipError
    b50 = A.TrainBatchBuilder(PPYOLO_2x_Config())
    pixels = lambda n: torch.from_numpy(np.ascontiguousarray(F.golden()['bgr_' + n])).cuda()
    want = {k: v.clone() for k, v in b50(_records(lambda n: dict(image=pixels(n))), 64, np.random.RandomState(17)).items()}
    got = b50.from_files(_records(lambda n: dict(image=F.data(n))), 64, np.random.RandomState(17), decoder=dec)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    with pytest.raises(PPYoloHipError, match='record 0: unsupported JPEG'):            # the builder's own decoder keeps the default
        b50.from_files(_records(lambda n: dict(image=F.data(n))), 64, np.random.RandomState(17))


def test_detect_files_equals_detect_raw(dec):
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = 320
    model, _ = build_model(cfg, 0, 'cuda')
    det = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
    got = det.detect_files([F.data(n) for n in _PAIR], decoder=dec)
    tensors = dec.decode([F.data(n) for n in _PAIR])
    assert all(F.matches_golden(n, t.cpu().numpy()) for n, t in zip(_PAIR, tensors))
    want = det.detect_raw(tensors)
    assert len(got) == len(want) == len(_PAIR)
    for n, g, w in zip(_PAIR, got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and np.array_equal(a, b), n
