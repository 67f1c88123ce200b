"""The training-batch kernels (csrc/augment.hip canvas_px / color_px / render_px) on the hand recipes of tests/augment_cases.py
(tests/test_augment_cases.py checks on the CPU that each recipe reaches what its name says): every colour-op order, the expand
wrap at values below 0 and beyond 512, mixup coverage and the float32 blend, one-pixel crops, the resize modes on windows inside
a striped canvas and on 1 x 1 ... 2 x 2 canvases, 8-bit accumulators beyond [0, 255].  The reference is tests/augment_ref.py on
the same recipe; every comparison is np.array_equal with dtype and shape.  The one exception is the one of
test_gpu_augment.py::test_canvas_kernel_equals_the_reference: a hue-last float64 canvas may differ by one float64 ulp."""
import numpy as np
import pytest
import torch

import augment_cases as C
from config import PPYOLO_2x_Config
from ppyolo_hip import augment as A, ops

pytestmark = pytest.mark.gpu
FAMILIES = ['colour', 'expand', 'mixup', 'crop', 'render', 'overshoot']
_NO_TARGETS = (np.zeros(0, np.int64), np.zeros(0, np.float32), None, None, None)


@pytest.fixture(scope='module')
def b():
    return A.TrainBatchBuilder(PPYOLO_2x_Config())


@pytest.fixture(scope='module')
def lut(b):
    return torch.from_numpy(b.lut_np).cuda()


def _render(b, lut, recipes, S, to_rgb):
    """One launch over `recipes` into an output pre-filled with NaN -> device float32 [n, 3, S, S]."""
    blob, lay = A.pack_batch(recipes, to_rgb, *_NO_TARGETS)
    dev = torch.from_numpy(blob).cuda()
    out = torch.full((len(recipes), 3, S, S), float('nan'), device='cuda')
    ops.augment_render(dev, len(recipes), S, lut, b.mean, b.std, out, sources=lay['sources'])
    return out


_SINGLE = {}


def _single(b, lut, name):
    """The case rendered alone, computed once and shared (host float32 [3, S, S]; do not modify)."""
    if name not in _SINGLE:
        c = C.CASES[name]
        _SINGLE[name] = _render(b, lut, [c['recipe']], c['S'], c['to_rgb'])[0].cpu().numpy()
    return _SINGLE[name]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), 'values differ')


def _hue_last_f64(r):
    return bool(r['ops']) and r['ops'][-1][0] == A.OP_HUE and r['canvas_dtype'] == A.F64


@pytest.mark.parametrize('fam', FAMILIES)
def test_canvas_kernel_equals_the_restatement(b, fam):
    used = cases_used = 0
    for c in C.family(fam):
        r = c['recipe']
        got = b.canvas(r, to_rgb=c['to_rgb']).cpu().numpy()
        want = C.expected_canvas(c['name'])
        assert got.dtype == want.dtype and got.shape == want.shape, c['name']
        if np.array_equal(got, want):
            continue
        bad = got != want
        assert _hue_last_f64(r), '%s (not hue-last float64) differs at %d values' % (c['name'], int(bad.sum()))
        assert np.all(np.abs(got[bad] - want[bad]) <= np.spacing(np.abs(want[bad]))), c['name']
        used += int(bad.sum())
        cases_used += 1
    n_hue = sum(_hue_last_f64(c['recipe']) for c in C.family(fam))
    print('AUGMENT-EDGES canvas %s: %d cases, %d of them hue-last float64; the one-ulp exception was used by %d values in %d cases'
          % (fam, len(C.family(fam)), n_hue, used, cases_used))
    assert cases_used <= n_hue


@pytest.mark.parametrize('fam', FAMILIES)
def test_render_kernel_equals_the_restatement(b, lut, fam):
    for c in C.family(fam):
        got = _single(b, lut, c['name'])
        assert not np.isnan(got).any(), c['name']                   # every pixel of the pre-filled output was written
        _same(got, C.expected_image(c['name']), c['name'])


@pytest.mark.parametrize('key', sorted(C.batches()), ids=lambda k: 'S%d_%s' % (k[0], 'rgb' if k[1] else 'bgr'))
def test_one_launch_for_all_cases_equals_one_launch_per_case(b, lut, key):
    """blockIdx.z indexes the descriptors: uint8 / float32 / float64 canvases and all three resize modes in one launch; twice."""
    S, to_rgb = key
    names = C.batches()[key]
    recipes = [C.CASES[n]['recipe'] for n in names]
    first = _render(b, lut, recipes, S, to_rgb)
    again = _render(b, lut, recipes, S, to_rgb)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    got = first.cpu().numpy()
    for k, n in enumerate(names):
        _same(got[k], _single(b, lut, n), n)
        _same(got[k], C.expected_image(n), n)
    if to_rgb:                                                      # (the six bgr cases are mixup cases: uint8 only)
        assert len({C.CASES[n]['recipe']['canvas_dtype'] for n in names}) == 3


def _pitched_view(im):
    """big[3:3+h, 5:5+w] of a tensor 11 rows and 13 columns larger whose storage starts one byte into a buffer; the surroundings
    are 255 / 0 stripes, so a read outside the view shows."""
    h, w = im.shape[:2]
    raw = torch.empty(1 + (h + 11) * (w + 13) * 3, dtype=torch.uint8, device='cuda')
    raw[0::2] = 255
    raw[1::2] = 0
    big = raw[1:].view(h + 11, w + 13, 3)
    v = big[3:3 + h, 5:5 + w]
    v.copy_(torch.from_numpy(im))
    assert big.data_ptr() % 2 == 1 and v.stride() == ((w + 13) * 3, 3, 1) and not v.is_contiguous()
    return v


@pytest.mark.parametrize('name', ['render_window_cubic_u8_S40', 'render_window_flip_lanczos4_f32_S40', 'render_window_linear_f64_S40',
                                  'mixup_then_hue_expand_crop_flip'])
def test_external_pitched_unaligned_sources(b, lut, name):
    c = C.CASES[name]
    r = c['recipe']
    dev_r = dict(r, image=_pitched_view(r['image']), mix_image=None if r['mix_image'] is None else _pitched_view(r['mix_image']))
    blob, lay = A.pack_batch([dev_r], c['to_rgb'], *_NO_TARGETS)
    assert len(lay['sources']) == (1 if r['mix_image'] is None else 2)
    want_cv = C.expected_canvas(name)
    got_cv = b.canvas(dev_r, to_rgb=c['to_rgb']).cpu().numpy()
    assert got_cv.dtype == want_cv.dtype and got_cv.shape == want_cv.shape
    assert np.array_equal(got_cv, b.canvas(r, to_rgb=c['to_rgb']).cpu().numpy())           # the host-source canvas, bit for bit
    if not _hue_last_f64(r):
        _same(got_cv, want_cv, name)
    got = _render(b, lut, [dev_r], c['S'], c['to_rgb'])[0].cpu().numpy()
    _same(got, C.expected_image(name), name)
