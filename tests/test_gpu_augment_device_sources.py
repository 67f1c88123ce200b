"""Training batches from device-resident images and JPEG files (ppyolo_hip/augment.py, csrc/augment.hip).  The oracle is
the host-source path of the same builder -- pinned to the reference by tests/test_gpu_augment.py -- with the same seed: every
key of the batch must be equal bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_fixtures as F
from conftest import build_train_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from ppyolo_hip import augment as A, ops
from ppyolo_hip._lib import PPYoloHipError, lib
from ppyolo_hip.jpeg import JpegDecoder
from test_augment_plan import golden_batches
from test_gpu_augment import _recipe

pytestmark = pytest.mark.gpu


def _map_images(samples, fn):
    """fn(image, sample index, 0 image / 1 mixup partner) on every image of the batch; the records are copies."""
    out = []
    for i, s in enumerate(samples):
        s = dict(s, image=fn(s['image'], i, 0))
        if 'mixup' in s:
            s['mixup'] = dict(s['mixup'], image=fn(s['mixup']['image'], i, 1))
        out.append(s)
    return out


def _cuda(im, *_):
    return torch.from_numpy(im).cuda()


def _equal(got, want, what=''):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


_WANT = {}


def _host_batch(b, key, samples, S, seed):
    """The oracle, computed once per (config, batch) and shared."""
    if key not in _WANT:
        _WANT[key] = {k: v.clone() for k, v in b(samples, S, np.random.RandomState(seed)).items()}
    return _WANT[key]


@pytest.fixture(scope='module')
def g19(golden):
    return [(seed, samples) for seed, _, samples, _, _ in golden_batches(golden('g19_augment'))[:3]]


@pytest.fixture(scope='module')
def b50():
    return A.TrainBatchBuilder(PPYOLO_2x_Config())


def test_device_sources_give_the_host_sources_batch(g19, b50):
    for seed, samples in g19:
        want = _host_batch(b50, ('g19', seed), samples, 64, seed)
        assert set(want) == {'images', 'gt_bbox', 'gt_class', 'gt_score', 'target0', 'target1', 'target2'}
        got = b50(_map_images(samples, _cuda), 64, np.random.RandomState(seed))
        assert len(b50._keep[2]) >= len(samples)             # the sources are held beside the blob
        _equal(got, want, seed)


def test_mixed_batches(g19, b50):
    """Even samples on the device, odd ones numpy; then device image + numpy partner and the reverse."""
    n_cross = 0
    for seed, samples in g19:
        want = _host_batch(b50, ('g19', seed), samples, 64, seed)
        _equal(b50(_map_images(samples, lambda im, i, m: _cuda(im) if i % 2 == 0 else im), 64, np.random.RandomState(seed)),
               want, seed)
        cross = _map_images(samples, lambda im, i, m: _cuda(im) if (i + m) % 2 == 0 else torch.from_numpy(im))
        n_cross += sum('mixup' in s for s in cross)
        _equal(b50(cross, 64, np.random.RandomState(seed)), want, seed)
    assert n_cross >= 2


def test_pitched_unaligned_views(g19, b50):
    """Each source is big[3:3+h, 5:5+w] of a tensor 11 rows and 13 columns larger whose storage starts one byte into a
    buffer; the surroundings are 255 / 0 stripes, so a read outside the view shows."""
    def view(im, *_):
        h, w = im.shape[:2]
        raw = torch.empty(1 + (h + 11) * (w + 13) * 3, dtype=torch.uint8, device='cuda')
        raw[0::2] = 255
        raw[1::2] = 0
        big = raw[1:].view(h + 11, w + 13, 3)
        v = big[3:3 + h, 5:5 + w]
        v.copy_(torch.from_numpy(im))
        assert big.data_ptr() % 2 == 1
        assert v.stride() == ((w + 13) * 3, 3, 1) and not v.is_contiguous()
        return v
    for seed, samples in g19:
        want = _host_batch(b50, ('g19', seed), samples, 64, seed)
        _equal(b50(_map_images(samples, view), 64, np.random.RandomState(seed)), want, seed)


def _small_batch(seed, n, lo=(7, 9), hi=(40, 33), same=None):
    """n samples with mixup partners, sources lo .. hi pixels, one or two boxes each."""
    rng = np.random.RandomState(seed)

    def one(k, m):
        if same is not None:
            h, w = same
        elif k == 0:
            h, w = lo if m == 0 else hi
        else:
            h, w = int(rng.randint(lo[0], hi[0] + 1)), int(rng.randint(lo[1], hi[1] + 1))
        G = int(rng.randint(1, 3))
        x1, y1 = rng.uniform(0, w - 5, G), rng.uniform(0, h - 5, G)
        box = np.stack([x1, y1, x1 + rng.uniform(3, 4, G), y1 + rng.uniform(3, 4, G)], 1).astype(np.float32)
        return dict(image=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), h=h, w=w, gt_bbox=box,
                    gt_class=rng.randint(0, 80, (G, 1)).astype(np.int32), gt_score=np.ones((G, 1), np.float32),
                    is_crowd=np.zeros((G, 1), np.int32))
    out = []
    for k in range(n):
        s = one(k, 0)
        s['mixup'] = one(k, 1)
        out.append(s)
    return out


def test_one_tensor_in_three_places(b50):
    """The same tensor is the image of sample 0, the mixup partner of sample 1 and the image of sample 2."""
    samples = _small_batch(3, 3, same=(23, 31))
    shared = samples[0]['image']
    samples[1]['mixup']['image'] = shared
    samples[2]['image'] = shared
    want = b50(samples, 32, np.random.RandomState(8))
    t = _cuda(shared)
    dev = _map_images(samples, lambda im, i, m: t if im is shared else _cuda(im))
    assert dev[0]['image'] is dev[1]['mixup']['image'] is dev[2]['image']
    _equal(b50(dev, 32, np.random.RandomState(8)), want)


@pytest.mark.parametrize('cfgc', [PPYOLO_2x_Config, PPYOLO_r18vd_Config])
@pytest.mark.parametrize('n', [9, 17])
def test_more_sources_than_one_launch_carries(cfgc, n):
    """A launch carries 16 table entries and consecutive windows share one: 18 sources take two launches, 34 take three, so
    window boundaries fall inside the batch; with three (r50) and two (r18) target levels."""
    b = A.TrainBatchBuilder(cfgc())
    samples = _small_batch(n, n)
    want = b(samples, 32, np.random.RandomState(n))
    recipes = b.plan(samples, 32, np.random.RandomState(n))[0]
    n_src = len(A.pack_batch(_dev_recipes(recipes), True, np.zeros(0, np.int64), np.zeros(0, np.float32), None, None, None)[1]['sources'])
    assert n_src > 15 * (1 if n == 9 else 2) + 1, n_src         # (a partner is dropped only at a mixup factor of 0 or 1)
    assert len(want) == 4 + len(b.anchor_masks)
    _equal(b(_map_images(samples, _cuda), 32, np.random.RandomState(n)), want)


def _dev_recipes(recipes):
    return [dict(r, image=_cuda(r['image']), mix_image=None if r['mix_image'] is None else _cuda(r['mix_image'])) for r in recipes]


def test_canvas_of_device_source_recipes(b50):
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, size=(37, 29, 3)).astype(np.uint8)
    for dt, torch_dt in ((A.U8, torch.uint8), (A.F32, torch.float32), (A.F64, torch.float64)):
        want = b50.canvas(_recipe(img, 32, A.LINEAR, dt, flip=dt == A.F32))
        got = b50.canvas(_recipe(_cuda(img), 32, A.LINEAR, dt, flip=dt == A.F32))
        assert got.dtype == want.dtype == torch_dt and torch.equal(got, want), dt
    # a planned recipe with a mixup partner, expand and crop as drawn
    samples = _small_batch(6, 4)
    for r in b50.plan(samples, 32, np.random.RandomState(6))[0]:
        assert torch.equal(b50.canvas(_dev_recipes([r])[0]), b50.canvas(r))


def test_tensors_the_builder_accepts_and_refuses(b50):
    samples = _small_batch(2, 2)
    want = b50(samples, 32, np.random.RandomState(2))
    _equal(b50(_map_images(samples, lambda im, *_: torch.from_numpy(im)), 32, np.random.RandomState(2)), want)     # CPU tensors: host sources
    img = _cuda(samples[0]['image'])
    chw = img.permute(2, 0, 1).contiguous()
    for bad, word in ((img.float(), 'uint8'), (chw, 'uint8 image'), (chw.permute(1, 2, 0), 'contiguous'), (img[:, ::2], 'contiguous')):
        with pytest.raises(PPYoloHipError, match=word):
            b50(_map_images(samples, lambda im, i, m: bad if (i, m) == (0, 0) else im), 32, np.random.RandomState(2))
    _equal(b50(_map_images(samples, lambda im, i, m: img[:, ::2].contiguous() if (i, m) == (1, 1) else im), 32,
               np.random.RandomState(2)),
           b50(_map_images(samples, lambda im, i, m: np.ascontiguousarray(samples[0]['image'][:, ::2]) if (i, m) == (1, 1) else im),
               32, np.random.RandomState(2)))


def _c_level(b):
    """One planned sample with an external source, ready for the C entry point: (call(n_src, ptr, pitch, h, w, blob=None), the
    numpy blob, the expected output)."""
    rng = np.random.RandomState(12)
    img = rng.randint(0, 256, size=(19, 23, 3)).astype(np.uint8)
    S = 32
    t = _cuda(img)
    blob, lay = A.pack_batch([_recipe(t, S, A.LINEAR, A.U8)], True, np.zeros(0, np.int64), np.zeros(0, np.float32), None, None, None)
    assert lay['sources'] == [t]
    host_blob, _ = A.pack_batch([_recipe(img, S, A.LINEAR, A.U8)], True, np.zeros(0, np.int64), np.zeros(0, np.float32), None, None, None)
    lut = torch.from_numpy(b.lut_np).cuda()
    want = torch.empty((1, 3, S, S), device='cuda')
    ops.augment_render(torch.from_numpy(host_blob).cuda(), 1, S, lut, b.mean, b.std, want)
    ms = (ctypes.c_double * 6)(*(list(b.mean) + list(b.std)))
    keep = []

    def call(out, n_src, ptr, pitch, h, w, blob_np=blob):
        dev = torch.from_numpy(blob_np).cuda()
        keep.append(dev)
        return lib().ppy_augment_render_src_f32(dev.data_ptr(), dev.numel(), 1, S, lut.data_ptr(), ms, 1, out.data_ptr(), n_src,
                                                (ctypes.c_void_p * 1)(ptr), (ctypes.c_longlong * 1)(pitch), (ctypes.c_int * 1)(h),
                                                (ctypes.c_int * 1)(w), torch.cuda.current_stream().cuda_stream)
    return call, blob, want, t, S


def test_c_level_argument_checks(b50):
    call, blob, want, t, S = _c_level(b50)
    out = torch.full((1, 3, S, S), 5.0, device='cuda')
    assert call(out, 1, None, 69, 19, 23) != 0                   # null source pointer
    assert call(out, 1, t.data_ptr(), 68, 19, 23) != 0           # pitch < 3 * w
    assert call(out, 1, t.data_ptr(), 69, 0, 23) != 0 and call(out, 1, t.data_ptr(), 69, 19, -1) != 0
    assert call(out, -1, t.data_ptr(), 69, 19, 23) != 0
    L = lib()
    cv = torch.full((19, 23, 3), 5, dtype=torch.uint8, device='cuda')
    dev = torch.from_numpy(blob).cuda()
    s = torch.cuda.current_stream().cuda_stream
    one = lambda v, ty: (ty * 1)(v)
    assert L.ppy_augment_canvas_src(dev.data_ptr(), dev.numel(), 0, 19, 23, 0, cv.data_ptr(), 1, one(None, ctypes.c_void_p),
                                    one(69, ctypes.c_longlong), one(19, ctypes.c_int), one(23, ctypes.c_int), s) != 0
    assert L.ppy_augment_canvas_src(dev.data_ptr(), dev.numel(), 0, 19, 23, 0, cv.data_ptr(), 1, one(t.data_ptr(), ctypes.c_void_p),
                                    one(60, ctypes.c_longlong), one(19, ctypes.c_int), one(23, ctypes.c_int), s) != 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((cv == 5).all())
    # the control: the same call with the right table renders the sample, and the canvas is the source
    assert call(out, 1, t.data_ptr(), 69, 19, 23) == 0
    assert L.ppy_augment_canvas_src(dev.data_ptr(), dev.numel(), 0, 19, 23, 0, cv.data_ptr(), 1, one(t.data_ptr(), ctypes.c_void_p),
                                    one(69, ctypes.c_longlong), one(19, ctypes.c_int), one(23, ctypes.c_int), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(cv, t.flip(2))        # to_rgb


def test_c_level_descriptors_that_do_not_fit_the_table_are_skipped(b50):
    call, blob, want, t, S = _c_level(b50)
    out = torch.full((1, 3, S, S), 5.0, device='cuda')
    i64 = blob[:64].view(np.int64)
    assert i64[0] == 0 and i64[6] == 1
    for idx in (1, 16, 1 << 40, -1):                            # index >= n_src (also beyond a window, beyond int), negative
        bad = blob.copy()
        bad[:64].view(np.int64)[0] = idx
        assert call(out, 1, t.data_ptr(), 69, 19, 23, bad) == 0
    bad = blob.copy()
    bad[:64].view(np.int64)[6] = 2                              # not a flag value
    assert call(out, 1, t.data_ptr(), 69, 19, 23, bad) == 0
    # the table entry's extent disagrees with the descriptor's h0 / w0 (each way the memory named stays inside the tensor)
    assert call(out, 1, t.data_ptr(), 69, 18, 23) == 0
    assert call(out, 1, t.data_ptr(), 69, 19, 22) == 0
    # an external descriptor and no table at all: the parent's entry point
    dev = torch.from_numpy(blob).cuda()
    ops.augment_render(dev, 1, S, torch.from_numpy(b50.lut_np).cuda(), b50.mean, b50.std, out)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert call(out, 1, t.data_ptr(), 69, 19, 23) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)


_FILES = [('c444_37x53', 'c420_q16_45x61'), ('c422_37x53', None), ('c420_37x53', 'c444_q16big_20x27'), ('grey_29x43', None),
          ('orient6_21x13', None)]


def _file_records(image_of):
    rng = np.random.RandomState(15)

    def one(name):
        h, w = F.pixels(name).shape[:2]
        G = int(rng.randint(1, 3))
        x1, y1 = rng.uniform(0, w - 8, G), rng.uniform(0, h - 8, G)
        box = np.stack([x1, y1, x1 + rng.uniform(4, 7, G), y1 + rng.uniform(4, 7, G)], 1).astype(np.float32)
        r = dict(h=h + 1, w=w, gt_bbox=box, gt_class=rng.randint(0, 80, (G, 1)).astype(np.int32),
                 gt_score=np.ones((G, 1), np.float32), is_crowd=np.zeros((G, 1), np.int32))        # (h + 1: the annotation is corrected)
        r.update(image_of(name))
        return r
    out = []
    for a, m in _FILES:
        s = one(a)
        if m is not None:
            s['mixup'] = one(m)
        out.append(s)
    return out


@pytest.fixture(scope='module')
def files_want(b50):
    assert F.pixels('orient6_21x13').shape == (13, 21, 3)        # an EXIF orientation that transposes
    return {k: v.clone() for k, v in b50(_file_records(lambda n: dict(image=F.pixels(n))), 64, np.random.RandomState(15)).items()}


@pytest.mark.parametrize('entropy', ['host', 'device'])
def test_from_files_equals_the_builder_on_the_decoded_pixels(b50, files_want, entropy, tmp_path):
    dec = JpegDecoder(entropy=entropy)
    records = _file_records(lambda n: dict(image=F.data(n)))
    _equal(b50.from_files(records, 64, np.random.RandomState(15), decoder=dec), files_want, entropy)
    assert isinstance(records[0]['image'], bytes) and records[0]['h'] == 38          # the caller's records are as they were
    if entropy == 'host':           # once more from files on disk, through the builder's own decoder
        def on_disk(n):
            p = tmp_path / (n + '.jpg')
            p.write_bytes(F.data(n))
            return dict(im_file=str(p))
        _equal(b50.from_files(_file_records(on_disk), 64, np.random.RandomState(15)), files_want, 'im_file')


def test_refused_files(b50):
    refused = dict((kind, name) for name, kind in F.refused())
    prog, corrupt = refused['unsupported'], refused['corrupt']
    fixed = np.random.RandomState(16).randint(0, 256, (30, 30, 3)).astype(np.uint8)

    def records(image_of):
        recs = _file_records(image_of)[:3]
        recs[1] = dict(recs[1], **image_of(None))
        recs[1]['gt_bbox'] = np.array([[2, 3, 20, 25]], np.float32)
        for k in ('gt_class', 'gt_score', 'is_crowd'):
            recs[1][k] = recs[1][k][:1]
        return recs
    as_files = lambda n: dict(image=F.data(prog if n is None else n))
    with pytest.raises(PPYoloHipError, match='record 1: unsupported JPEG'):
        b50.from_files(records(as_files), 64, np.random.RandomState(16))
    want = b50(records(lambda n: dict(image=fixed if n is None else F.pixels(n))), 64, np.random.RandomState(16))
    _equal(b50.from_files(records(as_files), 64, np.random.RandomState(16), fallback=lambda data: fixed), want)
    with pytest.raises(PPYoloHipError, match='record 1: corrupt JPEG'):
        b50.from_files(records(lambda n: dict(image=F.data(corrupt if n is None else n))), 64, np.random.RandomState(16),
                       fallback=lambda data: fixed)


def test_sources_dropped_right_after_the_call(b50, files_want):
    """The decoder runs on a side stream, the builder on the current one; the caller drops every reference at once and the
    side stream allocates and fills tensors of the same sizes.  (Can pass by luck without record_stream; must pass with it.)"""
    want = files_want
    side = torch.cuda.Stream()
    dec = JpegDecoder()
    with torch.cuda.stream(side):
        recs = A.decode_records(_file_records(lambda n: dict(image=F.data(n))), dec)
    sizes = [tuple(r['image'].shape) for r in recs] + [tuple(r['mixup']['image'].shape) for r in recs if 'mixup' in r]
    torch.cuda.current_stream().wait_stream(side)
    got = b50(recs, 64, np.random.RandomState(15))
    del recs
    b50._keep = None
    with torch.cuda.stream(side):
        junk = [torch.full(s, 255, dtype=torch.uint8, device='cuda') for s in sizes * 4]
    torch.cuda.synchronize()
    assert len(junk) == 4 * len(sizes)
    _equal(got, want)


def test_reference_training_call_on_a_device_source_batch():
    cfg = PPYOLO_r18vd_Config()
    b = A.TrainBatchBuilder(cfg)
    m = build_train_model(cfg, 0, 'cuda')
    m.head.set_dropblock(is_test=True)
    samples = _small_batch(18, 2, lo=(30, 40), hi=(60, 50))
    host = b(samples, 320, np.random.RandomState(18))
    dev = b(_map_images(samples, _cuda), 320, np.random.RandomState(18))
    call = lambda d: m(d['images'], None, False, d['gt_bbox'], d['gt_class'], d['gt_score'], [d['target0'], d['target1']])
    l_host, l_dev = call(host), call(dev)
    assert sorted(l_host) == sorted(l_dev) and len(l_host) >= 5
    for k in l_host:
        assert torch.equal(l_dev[k].detach(), l_host[k].detach()), k
