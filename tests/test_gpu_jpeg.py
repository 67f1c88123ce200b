"""JPEG decoding on the device (csrc/jpeg.hip, ppyolo_hip/jpeg.py) against tests/jpeg_ref.py and the libjpeg-turbo pixels of
tests/golden/g20_jpeg.npz.  Array equality everywhere; Pillow is not needed."""
import numpy as np
import pytest
import torch

import jpeg_fixtures as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dec():
    from ppyolo_hip.jpeg import JpegDecoder
    return JpegDecoder()


@pytest.mark.parametrize('name', F.names())
def test_one_by_one(dec, name):
    got = dec.imdecode(F.data(name))
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
    got = got.cpu().numpy()
    assert got.shape == F.pixels(name).shape
    assert np.array_equal(got, F.pixels(name))
    assert F.matches_golden(name, got)


def test_mixed_batch(dec):
    """Every fixture in ONE call: different sizes, samplings, orientations, grey and colour."""
    names = F.names()
    outs = dec.decode([F.data(n) for n in names])
    assert len(outs) == len(names)
    for n, t in zip(names, outs):
        got = t.cpu().numpy()
        assert got.shape == F.pixels(n).shape and np.array_equal(got, F.pixels(n)) and F.matches_golden(n, got), n


def test_batch_of_memoryviews_and_paths(dec, tmp_path):
    names = ['c422_37x53', 'grey_29x43', 'coco_398725']
    p = tmp_path / 'a.jpg'
    p.write_bytes(F.data(names[0]))
    outs = dec.decode([str(p), memoryview(F.data(names[1])), bytearray(F.data(names[2]))])
    for n, t in zip(names, outs):
        assert np.array_equal(t.cpu().numpy(), F.pixels(n))
    assert np.array_equal(dec.imread(p).cpu().numpy(), F.pixels(names[0]))


def test_orientation_off():
    from ppyolo_hip.jpeg import JpegDecoder
    raw = JpegDecoder(apply_orientation=False)
    names = [n for n in F.names() if n.startswith('orient')]
    outs = raw.decode([F.data(n) for n in names])
    for n, t in zip(names, outs):
        got = t.cpu().numpy()
        assert got.shape == (21, 13, 3) and np.array_equal(got, F.pixels(n, oriented=False)), n
        assert F.matches_golden(n, got, oriented=False)
        assert np.array_equal(got, F.pixels('orient1_21x13'))


def test_row_stride(dec):
    """Rows of a wider buffer (row stride not 3 * w, rows not 4-byte aligned); the bytes outside the image stay untouched."""
    names = ['c420_37x53', 'orient6_21x13', 'c444_opt_q35_50x50', 'c420_1x1']
    wide, outs = [], []
    for i, n in enumerate(names):
        h, w, _ = F.pixels(n).shape
        big = torch.full((h, w + 3 + i, 3), 0xA5, dtype=torch.uint8, device='cuda')
        wide.append(big)
        outs.append(big[:, 1:1 + w])
    res = dec.decode([F.data(n) for n in names], out=outs)
    assert all(a is b for a, b in zip(res, outs))
    for n, big in zip(names, wide):
        h, w, _ = F.pixels(n).shape
        got = big.cpu().numpy()
        assert np.array_equal(got[:, 1:1 + w], F.pixels(n)), n
        assert np.all(got[:, :1] == 0xA5) and np.all(got[:, 1 + w:] == 0xA5), n
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError):
        dec.decode([F.data(names[0])], out=[torch.empty((37, 52, 3), dtype=torch.uint8, device='cuda')])


def test_repeatable(dec):
    names = F.names()
    datas = [F.data(n) for n in names]
    first = [t.cpu().numpy() for t in dec.decode(datas)]
    for _ in range(3):                     # both staging buffers come round
        again = dec.decode(datas)
        assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(first, again))


def test_threads_are_capped():
    from ppyolo_hip import jpeg
    d = jpeg.JpegDecoder(threads=64)
    assert d.threads == 16 and jpeg.MAX_THREADS == 16
    one = jpeg.JpegDecoder(threads=1)
    names = F.names()[:5]
    for n, t in zip(names, one.decode([F.data(n) for n in names])):
        assert np.array_equal(t.cpu().numpy(), F.pixels(n))
    assert one._pool is None


@pytest.mark.parametrize('name,kind', F.refused())
def test_refused_files_raise(dec, name, kind):
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError) as e:
        dec.imdecode(F.data(name))
    assert ('progressive' in str(e.value) and 'unsupported' in str(e.value)) if kind == 'unsupported' else 'corrupt' in str(e.value)
    with pytest.raises(PPYoloHipError) as e:          # inside a batch the message names the item
        dec.decode([F.data('c420_37x53'), F.data(name)])
    assert 'item 1' in str(e.value)


def test_host_batches_own_their_staging_buffer():
    """A HostBatch keeps its pinned buffer until it is reconstructed or released: a third waiting batch is refused, not
    allowed to overwrite the first, and a batch whose buffer has moved on is refused too."""
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.jpeg import JpegDecoder
    d = JpegDecoder()
    a = d.entropy_decode([F.data('c420_37x53')])
    b = d.entropy_decode([F.data('grey_29x43')])
    with pytest.raises(PPYoloHipError) as e:
        d.entropy_decode([F.data('c444_37x53')])
    assert 'two batches ahead' in str(e.value)
    assert np.array_equal(d.reconstruct(b)[0].cpu().numpy(), F.pixels('grey_29x43'))
    with pytest.raises(PPYoloHipError) as e:               # a refused file gives its buffer back
        d.entropy_decode([F.data('truncated_c420_37x53')])
    assert 'corrupt' in str(e.value)
    assert np.array_equal(d.reconstruct(a)[0].cpu().numpy(), F.pixels('c420_37x53'))
    assert np.array_equal(d.reconstruct(a)[0].cpu().numpy(), F.pixels('c420_37x53'))          # again, while it is still the buffer's batch
    c = d.entropy_decode([F.data('c444_37x53')])
    d.release(c)
    e1 = d.entropy_decode([F.data('c422_37x53')])
    e2 = d.entropy_decode([F.data('c420_5x5')])
    stale = [h for h in (a, b, c) if (h.slot, h.gen) not in ((e1.slot, e1.gen), (e2.slot, e2.gen))]
    assert len(stale) == 3
    with pytest.raises(PPYoloHipError) as e:
        d.reconstruct(a)
    assert 'stale' in str(e.value)
    assert np.array_equal(d.reconstruct(e2)[0].cpu().numpy(), F.pixels('c420_5x5'))
    assert np.array_equal(d.reconstruct(e1)[0].cpu().numpy(), F.pixels('c422_37x53'))


def test_refused_outputs_give_their_staging_buffer_back():
    """decode() with an `out=` that reconstruct() refuses: the batch never reached the device, so its buffer is free again.
    Three refusals in a row (there are two buffers), then three good decodes, so both buffers come round."""
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.jpeg import JpegDecoder
    d = JpegDecoder()
    data, want = F.data('c420_5x5'), F.pixels('c420_5x5')
    for shape in ((5, 4, 3), (4, 5, 3), (5, 5, 4)):
        with pytest.raises(PPYoloHipError, match=r'output 0 must be a uint8 device tensor \[5, 5, 3\]'):
            d.decode([data], out=[torch.empty(shape, dtype=torch.uint8, device='cuda')])
    for _ in range(3):
        got = d.decode([data])[0].cpu().numpy()
        assert np.array_equal(got, want) and F.matches_golden('c420_5x5', got)


def test_max_pixels():
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.jpeg import JpegDecoder
    small = JpegDecoder(max_pixels=37 * 53 - 1)
    with pytest.raises(PPYoloHipError) as e:
        small.imdecode(F.data('c420_37x53'))
    assert 'max_pixels' in str(e.value)
    assert np.array_equal(JpegDecoder(max_pixels=37 * 53).imdecode(F.data('c420_37x53')).cpu().numpy(), F.pixels('c420_37x53'))


def test_detect_files_equals_detect_raw():
    """Decode.detect_files(files) == Decode.detect_raw(the golden pixels of those files), exactly."""
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = 320
    model, _ = build_model(cfg, 0, 'cuda')
    dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
    names = F.names()
    got = dec.detect_files([F.data(n) for n in names])
    want = dec.detect_raw([F.pixels(n) for n in names])
    assert len(got) == len(want) == len(names)
    for n, g, w in zip(names, got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and np.array_equal(a, b), n
