"""Pillow's resize, host side (no GPU): the numpy restatement (tests/pil_resize_ref.py) equals the installed Pillow and the
golden, and the library's planner (ppy_pil_resize_plan, csrc/pil_resize.hip) writes the restatement's tables integer for
integer.  Pillow is imported plainly: without it the pin fails, it does not skip."""
import os

import numpy as np
import pytest
from PIL import Image

import pil_resize_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('random', 'binary')


@pytest.fixture(scope='module')
def g25():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g25_pil_resize.npz'))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import resize
    return resize


def sweep_pairs():
    rng = np.random.RandomState(25)
    return [((int(rng.randint(1, 91)), int(rng.randint(1, 91))), (int(rng.randint(1, 71)), int(rng.randint(1, 71)))) for _ in range(200)]


def pillow(img, ow, oh, f):
    return np.asarray(Image.fromarray(img).resize((ow, oh), f))


# ---- the restatement against Pillow and the golden ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.SMALL_CASES, ids=lambda c: '%dx%d_to_%dx%d' % (c[0] + c[1]))
def test_restatement_equals_pillow_and_golden(case, g25):
    (h, w), (ow, oh) = case
    for kind in KINDS:
        key = '%dx%d_%dx%d_%s' % (h, w, ow, oh, kind)
        img = ref.content(h, w, kind, ref.case_seed(h, w, ow, oh))
        assert np.array_equal(img, g25['in_' + key])
        for f in ref.FILTERS:
            got = ref.resize(img, ow, oh, f)
            assert got.shape == (oh, ow, 3)
            assert np.array_equal(got, g25['out_%s_f%d' % (key, f)]), (key, ref.NAMES[f], 'golden')
            assert np.array_equal(got, pillow(img, ow, oh, f)), (key, ref.NAMES[f], 'installed Pillow')


@pytest.mark.parametrize('f', ref.FILTERS, ids=lambda f: ref.NAMES[f])
def test_restatement_long_taps(f):
    (h, w), (ow, oh) = ref.LONG_CASE
    for kind in KINDS:
        img = ref.content(h, w, kind, 3)
        assert np.array_equal(ref.resize(img, ow, oh, f), pillow(img, ow, oh, f)), kind


@pytest.mark.parametrize('f', (ref.BICUBIC, ref.LANCZOS), ids=lambda f: ref.NAMES[f])
def test_restatement_coco_size(f):
    (h, w), (ow, oh) = ref.COCO_CASE
    for kind in KINDS:
        img = ref.content(h, w, kind, 4)
        assert np.array_equal(ref.resize(img, ow, oh, f), pillow(img, ow, oh, f)), kind


def test_restatement_sweep():
    """200 seeded size pairs, sides 1..90 to 1..70, all six filters, content alternating random / binary."""
    for i, ((h, w), (ow, oh)) in enumerate(sweep_pairs()):
        img = ref.content(h, w, KINDS[i & 1], 1000 + i)
        for f in ref.FILTERS:
            assert np.array_equal(ref.resize(img, ow, oh, f), pillow(img, ow, oh, f)), (h, w, ow, oh, ref.NAMES[f])


def test_hamming_constants_are_float_literals():
    """Resample.c writes the window as 0.54f + 0.46f * cos: with the double constants 21 -> 7 rounds one coefficient elsewhere,
    and Pillow's pixels tell the two apart."""
    assert ref.F054 != 0.54 and ref.F046 != 0.46
    k = ref.axis_table(21, 7, ref.HAMMING)[2]
    assert int(np.abs(k).sum()) > 0
    rng = np.random.RandomState(0)
    for _ in range(20):
        img = rng.randint(0, 256, (40, 21, 3)).astype(np.uint8)
        assert np.array_equal(ref.resize(img, 7, 40, ref.HAMMING), pillow(img, 7, 40, ref.HAMMING))


# ---- the library's planner against the restatement ---------------------------------------------------------------------------
def expect_axis(insz, outsz, f):
    """What the planner must write for one axis: (ksize, kind, bounds, k)."""
    if insz == outsz:
        return 0, -1, np.stack([np.arange(outsz), np.ones(outsz, int)], 1), np.zeros((outsz, 0), int)
    if f == ref.NEAREST:
        return 0, 0, np.stack([ref.nearest_map(insz, outsz), np.ones(outsz, int)], 1), np.zeros((outsz, 0), int)
    ksize, bounds, k = ref.axis_table(insz, outsz, f)
    return ksize, f, bounds, k


def check_axis(table, insz, outsz, f):
    ksize, kind, bounds, k = expect_axis(insz, outsz, f)
    assert (table['insz'], table['outsz'], table['ksize'], table['kind']) == (insz, outsz, ksize, kind)
    assert np.array_equal(table['bounds'], bounds)
    assert np.array_equal(table['k'], k)


def check_plan(lib, h, w, ow, oh, f):
    blob, ws_bytes = lib.plan_host([(h, w)], ow, oh, f)
    p = lib.parse_plan(blob)
    assert p['magic'] == b'PIL1' and (p['n'], p['ow'], p['oh'], p['filter']) == (1, ow, oh, f)
    assert p['blob_bytes'] == blob.size and p['ws_bytes'] == ws_bytes
    im = p['images'][0]
    assert (im['h'], im['w']) == (h, w)
    if w == ow:
        assert im['xtab'] == -1 and ws_bytes == 0 and p['max_h_horizontal'] == 0
    else:
        check_axis(p['tables'][im['xtab']], w, ow, f)
        assert p['mid_pitch'] >= 3 * ow and p['mid_pitch'] % 16 == 0 and ws_bytes >= h * p['mid_pitch'] and p['max_h_horizontal'] == h
    check_axis(p['tables'][im['ytab']], h, oh, f)


@pytest.mark.parametrize('f', ref.FILTERS, ids=lambda f: ref.NAMES[f])
def test_planner_tables_case_list(lib, f):
    cases = ref.SMALL_CASES + [ref.LONG_CASE, ref.COCO_CASE, ((375, 500), (416, 416))]
    for (h, w), (ow, oh) in cases:
        check_plan(lib, h, w, ow, oh, f)


def test_planner_tables_long_lanczos(lib):
    check_plan(lib, 2160, 3840, 608, 608, ref.LANCZOS)
    assert ref.ksize_of(3840, 608, ref.LANCZOS) == 39
    check_plan(lib, 1080, 1920, 64, 64, ref.LANCZOS)
    assert ref.ksize_of(1920, 64, ref.LANCZOS) == 181


def test_planner_tables_sweep(lib):
    for (h, w), (ow, oh) in sweep_pairs():
        for f in ref.FILTERS:
            check_plan(lib, h, w, ow, oh, f)


def test_planner_shares_tables_within_a_batch(lib):
    sizes = [(480, 640), (480, 640), (375, 500), (640, 480), (608, 608)]
    blob, ws_bytes = lib.plan_host(sizes, 608, 608, ref.BICUBIC)
    p = lib.parse_plan(blob)
    im = p['images']
    # distinct axes: 640, 480, 500, 375 -> 608, and the identity map of the image that keeps its height
    assert p['n_tables'] == 5 and len(p['tables']) == 5
    assert (im[0]['xtab'], im[0]['ytab']) == (im[1]['xtab'], im[1]['ytab'])
    assert im[3]['xtab'] == im[0]['ytab'] and im[3]['ytab'] == im[0]['xtab']          # 480 -> 608 and 640 -> 608, either axis
    assert im[4]['xtab'] == -1 and p['tables'][im[4]['ytab']]['kind'] == -1
    for i, (h, w) in enumerate(sizes):
        if w != 608:
            check_axis(p['tables'][im[i]['xtab']], w, 608, ref.BICUBIC)
        check_axis(p['tables'][im[i]['ytab']], h, 608, ref.BICUBIC)
    # the intermediates: one per image that runs the horizontal pass, disjoint, inside the workspace
    mids = sorted((im[i]['mid_offset'], sizes[i][0] * p['mid_pitch']) for i in range(4))
    for (a, n), (b, _) in zip(mids, mids[1:]):
        assert a + n <= b
    assert mids[-1][0] + mids[-1][1] <= ws_bytes and p['max_h_horizontal'] == 640
    # the same batch of equal sizes needs exactly two tables
    assert lib.parse_plan(lib.plan_host([(480, 640)] * 8, 608, 608, ref.LANCZOS)[0])['n_tables'] == 2


@pytest.mark.parametrize('sizes,ow,oh,f,word', [
    ([(65536, 10)], 16, 16, 3, '65536'),
    ([(10, 65536)], 16, 16, 3, '65536'),
    ([(0, 10)], 16, 16, 3, 'input size'),
    ([(10, 10)], 8193, 16, 3, '8193'),
    ([(10, 10)], 16, 8193, 3, '8193'),
    ([(10, 10)], 0, 16, 3, 'output size'),
    ([(10, 10), (65535, 10)], 16, 64, 1, 'ksize 6145'),       # lanczos: ceil(3 * 65535 / 64) * 2 + 1
    ([(10, 65535)], 64, 16, 1, 'ksize 6145'),
])
def test_planner_refuses_by_name(lib, sizes, ow, oh, f, word):
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError) as e:
        lib.plan_host(sizes, ow, oh, f)
    assert word in str(e.value)


def test_planner_limits_are_inclusive(lib):
    lib.plan_host([(65535, 1)], 1, 8192, ref.NEAREST)
    # ksize 1023 passes: bilinear, 511 * out <= in < 511.x * out
    assert ref.ksize_of(511, 1, ref.BILINEAR) == 1023
    lib.plan_host([(511, 511)], 1, 1, ref.BILINEAR)
    assert ref.ksize_of(513, 1, ref.BILINEAR) == 1027
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError):
        lib.plan_host([(513, 513)], 1, 1, ref.BILINEAR)


def test_filter_codes_refused_by_name(lib):
    from ppyolo_hip._lib import PPYoloHipError
    for bad in (6, -1, 2.0, 'bicubic', True, None):
        with pytest.raises(PPYoloHipError) as e:
            lib.check_filter(bad)
        assert repr(bad) in str(e.value)
    assert [lib.NEAREST, lib.LANCZOS, lib.BILINEAR, lib.BICUBIC, lib.BOX, lib.HAMMING] == [
        Image.Resampling.NEAREST, Image.Resampling.LANCZOS, Image.Resampling.BILINEAR, Image.Resampling.BICUBIC,
        Image.Resampling.BOX, Image.Resampling.HAMMING]


def _cfg(**resize):
    from config import PPYOLO_2x_Config
    cfg = PPYOLO_2x_Config()
    cfg.resizeImage = dict(cfg.resizeImage, **resize)
    return cfg


def test_preprocessor_reads_the_switch(lib):
    """Construction is host work (device='cpu' holds the table on the host): the switch, the codes and the refusals."""
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.preprocess import Preprocessor
    assert Preprocessor(_cfg(), 608, 'cpu')._pil is None                                    # shipped: cv2 cubic
    assert Preprocessor(_cfg(use_cv2=True), 608, 'cpu')._pil is None
    assert Preprocessor(_cfg(use_cv2=False), 608, 'cpu')._pil.filter == lib.BILINEAR          # interp=2 is Pillow's BILINEAR
    for code in range(6):
        assert Preprocessor(_cfg(use_cv2=False, interp=code), 608, 'cpu')._pil.filter == code
    for bad in (6, -1, 'cubic'):
        with pytest.raises(PPYoloHipError) as e:
            Preprocessor(_cfg(use_cv2=False, interp=bad), 608, 'cpu')
        assert repr(bad) in str(e.value)
    with pytest.raises(PPYoloHipError) as e:
        Preprocessor(_cfg(use_cv2='no'), 608, 'cpu')
    assert "'no'" in str(e.value)
    with pytest.raises(PPYoloHipError):                                                     # cv2 branch: still cubic only
        Preprocessor(_cfg(interp=1), 608, 'cpu')
    for kw in (dict(max_size=1333), dict(max_size=1333, use_cv2=False, interp=3)):
        with pytest.raises(PPYoloHipError) as e:
            Preprocessor(_cfg(**kw), 608, 'cpu')
        assert 'max_size=1333' in str(e.value)
