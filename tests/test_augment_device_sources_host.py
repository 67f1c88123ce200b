"""Device-resident sources of the training-batch builder, the host half (ppyolo_hip/augment.py): the planner takes tensors
and draws as it does for numpy images; pack_batch puts no pixel of an external source into the blob and packs numpy
records as it always did; decode_records is the reference's DecodeImage for a batch, through one decoder call."""
import copy

import numpy as np
import pytest
import torch

from config import PPYOLO_2x_Config
from ppyolo_hip import augment as A
from ppyolo_hip._lib import PPYoloHipError
from test_augment_plan import golden_batches, plan_batch


def _with_images(samples, fn):
    out = []
    for s in samples:
        s = dict(s, image=fn(s['image']))
        if 'mixup' in s:
            s['mixup'] = dict(s['mixup'], image=fn(s['mixup']['image']))
        out.append(s)
    return out


def _strip(r):
    return {k: v for k, v in r.items() if k not in ('image', 'mix_image')}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) == type(b) and a == b


def test_planner_takes_tensors_and_draws_the_same(golden):
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    for seed, shape, samples, _, _ in golden_batches(golden('g19_augment'))[:3]:
        _, (r0, bb0, cl0, sc0) = plan_batch(b, seed, samples)
        st0 = np.random.get_state()
        _, (r1, bb1, cl1, sc1) = plan_batch(b, seed, _with_images(samples, torch.from_numpy))
        st1 = np.random.get_state()
        assert np.array_equal(st0[1], st1[1]) and st0[2:] == st1[2:], seed
        assert len(r0) == len(r1)
        for x, y in zip(r0, r1):
            assert _same(_strip(x), _strip(y)), seed
            assert isinstance(y['image'], np.ndarray) and np.array_equal(x['image'], y['image'])     # a CPU tensor is the array it wraps
            assert (x['mix_image'] is None) == (y['mix_image'] is None)
        assert _same(bb0, bb1) and _same(cl0, cl1) and _same(sc0, sc1), seed


def _external(im):
    """A stand-in for a device tensor on a box without one: pack_batch's rule (augment.is_external) is `a tensor that is not in
    host memory`, which a meta tensor of the image's shape satisfies."""
    return torch.empty(im.shape, dtype=torch.uint8, device='meta')


def test_external_sources_put_no_pixels_into_the_blob(golden):
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    for seed, shape, samples, _, _ in golden_batches(golden('g19_augment'))[:3]:
        _, (recipes, bb, cl, sc) = plan_batch(b, seed, samples)
        host, lay_h = A.pack_batch(recipes, True, np.zeros(3, np.int64), np.zeros(3, np.float32), bb, cl, sc)
        ext = [dict(r, image=_external(r['image']), mix_image=None if r['mix_image'] is None else _external(r['mix_image']))
               for r in recipes]
        assert all(A.is_external(r['image']) for r in ext)
        dev, lay_d = A.pack_batch(ext, True, np.zeros(3, np.int64), np.zeros(3, np.float32), bb, cl, sc)
        srcs = lay_d['sources']
        n_src = len(recipes) + sum(r['mix_image'] is not None for r in recipes)
        assert len(srcs) == n_src and n_src > len(recipes)
        pixels = sum(int(t.shape[0]) * int(t.shape[1]) * 3 for t in srcs)
        assert len(dev) <= len(host) - pixels + 64 * n_src
        # descriptors: still DESC_BYTES each at offset 0; the table order is sample order, a sample's two sources adjacent
        assert A.DESC_BYTES == 328 and lay_d['desc'] == 0 and lay_d['toff'] >= A.DESC_BYTES * len(recipes)
        k = 0
        for i, r in enumerate(ext):
            d = dev[i * A.DESC_BYTES:(i + 1) * A.DESC_BYTES]
            i64 = d[:64].view(np.int64)
            i32 = d[64 + 8 * A.DESC_F64:64 + 8 * A.DESC_F64 + 4 * A.DESC_I32].view(np.int32)
            assert i64[0] == k and i64[6] == 1 and srcs[k] is r['image'] and tuple(i32[:2]) == tuple(r['image'].shape[:2])
            k += 1
            if r['mix_image'] is not None:
                assert i64[1] == k and i64[7] == 1 and srcs[k] is r['mix_image'] and tuple(i32[2:4]) == tuple(r['mix_image'].shape[:2])
                k += 1
            else:
                assert i64[1] == 0 and i64[7] == 0
        # everything but the pixels and the descriptors' source fields is what the host blob carries
        for key in ('gt_bbox', 'gt_class', 'gt_score'):
            n = {'gt_bbox': bb, 'gt_class': cl, 'gt_score': sc}[key].nbytes
            assert np.array_equal(dev[lay_d[key]:lay_d[key] + n], host[lay_h[key]:lay_h[key] + n])


def test_numpy_records_pack_as_before(golden):
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    seed, shape, samples, _, _ = golden_batches(golden('g19_augment'))[0]
    _, (recipes, bb, cl, sc) = plan_batch(b, seed, samples)
    toff, tval = np.arange(5, dtype=np.int64), np.arange(5, dtype=np.float32)
    blob, lay = A.pack_batch(recipes, True, toff, tval, bb, cl, sc)
    blob2, lay2 = A.pack_batch(recipes, True, toff, tval, bb, cl, sc)
    assert lay['sources'] == [] and np.array_equal(blob, blob2) and blob.dtype == np.uint8
    assert {k: v for k, v in lay.items() if k != 'sources'} == {k: v for k, v in lay2.items() if k != 'sources'}
    assert set(lay) == {'desc', 'toff', 'tval', 'gt_bbox', 'gt_class', 'gt_score', 'sources'}
    # the descriptor's two new fields are the parent's spare zeros, and every source lies in the blob, rows packed
    pos = A.DESC_BYTES * len(recipes)
    for i, r in enumerate(recipes):
        i64 = blob[i * A.DESC_BYTES:i * A.DESC_BYTES + 64].view(np.int64)
        assert i64[6] == 0 and i64[7] == 0
        pos = (pos + 15) // 16 * 16
        assert i64[0] == pos, i
        n = r['image'].size
        assert np.array_equal(blob[pos:pos + n], r['image'].ravel())
        pos += n
        if r['mix_image'] is not None:
            pos = (pos + 15) // 16 * 16
            assert i64[1] == pos
            pos += r['mix_image'].size
        for t in ('xfirst', 'xw', 'yfirst', 'yw'):
            pos = (pos + 15) // 16 * 16 + r['resize'][t].size * 4
    # a CPU tensor packs as the array it wraps
    blob3, lay3 = A.pack_batch([dict(r, image=torch.from_numpy(r['image'])) for r in recipes], True, toff, tval, bb, cl, sc)
    assert lay3['sources'] == [] and np.array_equal(blob, blob3)


class _StubDecoder(object):
    """decode(items) -> CPU tensors whose shape the first two bytes name; refusal() refuses by the third byte."""

    def __init__(self, with_refusal=True):
        self.calls = []
        if not with_refusal:
            self.refusal = None

    def refusal(self, data):
        return {1: ('unsupported', 'progressive JPEG'), 2: ('corrupt', 'truncated')}.get(data[2])

    def decode(self, items):
        self.calls.append(list(items))
        for k, d in enumerate(items):
            if d[2] == 3:           # damage the header pass cannot see
                raise PPYoloHipError('item %d: corrupt JPEG: bad Huffman code (code -5)' % k)
        return [torch.full((d[0], d[1], 3), d[3], dtype=torch.uint8) for d in items]


def _rec(image=None, im_file=None, h=1, w=1, **kw):
    r = dict(h=h, w=w, gt_bbox=np.zeros((1, 4), np.float32), gt_class=np.zeros((1, 1), np.int32),
             gt_score=np.ones((1, 1), np.float32), is_crowd=np.zeros((1, 1), np.int32), **kw)
    if image is not None:
        r['image'] = image
    if im_file is not None:
        r['im_file'] = im_file
    return r


def test_decode_records_with_a_stub_decoder(tmp_path):
    f = tmp_path / 'a.jpg'
    f.write_bytes(bytes([9, 8, 0, 77]))
    ready = np.zeros((4, 5, 3), np.uint8)
    records = [_rec(image=bytes([6, 7, 0, 11]), h=600, w=700, mixup=_rec(image=bytes([3, 4, 0, 22]))),
               _rec(image=ready, h=4, w=5),                                         # decoded already: left alone
               _rec(im_file=str(f), mixup=_rec(image=ready, h=4, w=5))]             # no 'image': the file is read; no h / w fix needed
    before = copy.deepcopy(records)
    dec = _StubDecoder()
    out = A.decode_records(records, dec)
    assert len(dec.calls) == 1 and dec.calls[0] == [bytes([6, 7, 0, 11]), bytes([3, 4, 0, 22]), bytes([9, 8, 0, 77])]
    assert [tuple(o['image'].shape) for o in out] == [(6, 7, 3), (4, 5, 3), (9, 8, 3)]
    assert (out[0]['h'], out[0]['w']) == (6, 7) and (out[2]['h'], out[2]['w']) == (9, 8)        # corrected / set
    assert tuple(out[0]['mixup']['image'].shape) == (3, 4, 3) and (out[0]['mixup']['h'], out[0]['mixup']['w']) == (3, 4)
    assert int(out[0]['image'][0, 0, 0]) == 11 and int(out[2]['image'][0, 0, 0]) == 77
    assert out[1]['image'] is ready and out[2]['mixup']['image'] is ready
    # the caller's records are as they were
    assert _same(records, before) and isinstance(records[0]['image'], bytes) and 'image' not in records[2]
    assert isinstance(records[0]['mixup']['image'], bytes) and records[0]['h'] == 600
    # without mixup the partners are neither decoded nor touched
    dec = _StubDecoder()
    out = A.decode_records(records, dec, with_mixup=False)
    assert dec.calls == [[bytes([6, 7, 0, 11]), bytes([9, 8, 0, 77])]] and isinstance(out[0]['mixup']['image'], bytes)
    # the planner takes the result (CPU tensors are host sources)
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    recipes = b.plan(A.decode_records(records, _StubDecoder()), 320, np.random.RandomState(0))[0]
    assert len(recipes) == 3


def test_decode_records_refusals(tmp_path):
    f = tmp_path / 'p.jpg'
    f.write_bytes(bytes([2, 2, 1, 0]))
    records = [_rec(image=bytes([6, 7, 0, 11])), _rec(im_file=str(f)), _rec(image=bytes([5, 5, 0, 33]))]
    dec = _StubDecoder()
    with pytest.raises(PPYoloHipError, match=r'record 1 .*p\.jpg.*unsupported.*progressive'):
        A.decode_records(records, dec)
    assert dec.calls == []                                   # found before anything was decoded
    fixed = np.full((2, 3, 3), 9, np.uint8)
    seen = []
    out = A.decode_records(records, dec, fallback=lambda data: seen.append(data) or fixed)
    assert seen == [bytes([2, 2, 1, 0])] and out[1]['image'] is fixed and (out[1]['h'], out[1]['w']) == (2, 3)
    assert dec.calls == [[bytes([6, 7, 0, 11]), bytes([5, 5, 0, 33])]]         # the good ones once, without the refused one
    assert tuple(out[2]['image'].shape) == (5, 5, 3)
    with pytest.raises(PPYoloHipError, match='fallback must return'):
        A.decode_records(records, _StubDecoder(), fallback=lambda data: fixed.astype(np.float32))
    # a corrupt file is an error with or without a fallback: seen by the header pass ...
    bad = [_rec(image=bytes([6, 7, 0, 11])), _rec(image=bytes([6, 7, 0, 11]), mixup=_rec(image=bytes([1, 1, 2, 0])))]
    with pytest.raises(PPYoloHipError, match=r"record 1\['mixup'\].*corrupt.*truncated"):
        A.decode_records(bad, _StubDecoder(), fallback=lambda data: fixed)
    # ... or only by the decode itself, whose item index is mapped back to the record
    late = [_rec(image=np.zeros((2, 2, 3), np.uint8)), _rec(image=bytes([6, 7, 0, 11])), _rec(image=bytes([4, 4, 3, 0]))]
    with pytest.raises(PPYoloHipError, match=r'record 2: corrupt JPEG: bad Huffman'):
        A.decode_records(late, _StubDecoder(), fallback=lambda data: fixed)
    with pytest.raises(PPYoloHipError, match=r'record 2: corrupt JPEG'):
        A.decode_records(late, _StubDecoder(with_refusal=False))
    with pytest.raises(PPYoloHipError, match='neither an image nor an im_file'):
        A.decode_records([_rec()], _StubDecoder())


def test_unusable_tensors_are_refused_with_the_reason():
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    im = torch.zeros((8, 6, 3), dtype=torch.uint8)
    assert isinstance(A.source_image(im, b.device), np.ndarray)
    assert A.source_image(im[:, ::2], b.device).shape == (8, 3, 3)          # host memory: packed by value, any strides
    for bad, word in ((im.float(), 'uint8'), (im[0], 'uint8 image'), (_external(np.zeros((8, 6, 3))), 'lives on')):
        with pytest.raises(PPYoloHipError, match=word):
            b.plan([_rec(image=bad)], 320)
