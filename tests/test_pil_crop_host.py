"""The crop entries, host side (no GPU): ppy_pil_crop_plan_bytes refuses every batch outside its limits by name and returns the
workspace formula of include/ppyolo_hip.h; PilResizer(box=) refuses on the host the two boxes Pillow refuses."""
import ctypes

import numpy as np
import pytest

import pil_resize_ref as ref


@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import ops
    return ops


def plan(ops, sizes, form, rows_or_m, ow, oh, f, pad=0.0, top_k=1, pitch=None, base=8):
    descs = ops.pil_crop_descs([(base, 3 * w if pitch is None else pitch, h, w) for h, w in sizes])
    return ops.pil_crop_plan_bytes(descs, len(sizes), form, rows_or_m, ow, oh, f, pad, top_k)


def A(v, to=256):
    return (v + to - 1) // to * to


def expect_bytes(sizes, cap, ow, oh, f):
    max_h, max_w = max(s[0] for s in sizes), max(s[1] for s in sizes)
    kx = 0 if f == ref.NEAREST else ref.ksize_of(max_w, ow, f)
    ky = 0 if f == ref.NEAREST else ref.ksize_of(max_h, oh, f)
    return (A(32 * cap) + A(4 * cap) + A(4 * cap * ow * (2 + kx)) + A(4 * cap * oh * (2 + ky))
            + cap * A(max_h * A(3 * ow, 16))), (kx, ky)


@pytest.mark.parametrize('f', ref.FILTERS, ids=lambda f: ref.NAMES[f])
def test_workspace_formula(ops, f):
    for sizes, form, rows, ow, oh in (([(480, 640)] * 8, 0, 100, 128, 128), ([(37, 53), (200, 3), (64, 48)], 0, 7, 16, 9),
                                      ([(13, 9)], 1, 5, 32, 31), ([(1, 1)], 1, 1, 1, 1), ([(90, 1)], 0, 1, 8192, 1)):
        cap = len(sizes) * rows if form == 0 else rows
        assert plan(ops, sizes, form, rows, ow, oh, f) == expect_bytes(sizes, cap, ow, oh, f)


@pytest.mark.parametrize('kw,word', [
    (dict(sizes=[(65536, 700)]), '65536'),
    (dict(sizes=[(10, 65536)]), '65536'),
    (dict(sizes=[(10, 10), (0, 10)]), 'image 1: input size'),
    (dict(ow=8193), '8193'),
    (dict(oh=8193), '8193'),
    (dict(ow=0), 'output size'),
    (dict(sizes=[(700, 65535)], ow=64, f=1), 'ksize 6145'),        # lanczos: ceil(3 * 65535 / 64) * 2 + 1
    (dict(sizes=[(10, 10), (65535, 700)], oh=64, f=1), 'ksize 6145'),
    (dict(f=6), 'filter code 6'),
    (dict(f=-1), 'filter code -1'),
    (dict(sizes=[(10, 10), (1001, 10)]), 'image 1: 10 x 1001 is taller than 100 x its width'),
    (dict(sizes=[(10, 10)] * 2, rows_or_m=32769), '65538 candidates'),
    (dict(form=1, rows_or_m=65537), 'list of 65537'),
    (dict(form=1, rows_or_m=0), 'list of 0'),
    (dict(rows_or_m=0), '0 rows'),
    (dict(pad=-0.001), 'pad -0.001'),
    (dict(pad=4.5), 'pad 4.5'),
    (dict(pad=float('nan')), 'pad nan'),
    (dict(pad=float('inf')), 'pad inf'),
    (dict(top_k=0), 'top_k 0'),
])
def test_refused_by_name(ops, kw, word):
    from ppyolo_hip._lib import PPYoloHipError
    args = dict(sizes=[(10, 10)], form=0, rows_or_m=4, ow=16, oh=16, f=3, pad=0.0, top_k=1)
    args.update(kw)
    with pytest.raises(PPYoloHipError) as e:
        plan(ops, **args)
    assert word in str(e.value), str(e.value)


def test_limits_are_inclusive(ops):
    plan(ops, [(65535, 656)], 0, 1, 1, 8192, ref.NEAREST)
    plan(ops, [(1000, 10)], 0, 1, 4, 4, ref.BOX)                       # h == 100 * w passes
    plan(ops, [(10, 10)] * 2, 0, 32768, 1, 1, ref.NEAREST)             # n * K == 65536
    plan(ops, [(10, 10)], 1, 65536, 1, 1, ref.NEAREST)
    plan(ops, [(10, 10)], 0, 4, 8, 8, ref.BICUBIC, pad=4.0, top_k=1)
    plan(ops, [(10, 10)], 0, 4, 8, 8, ref.BICUBIC, pad=0.0)
    assert ref.ksize_of(511, 1, ref.BILINEAR) == 1023                  # ksize 1023 passes, 1027 does not
    assert plan(ops, [(511, 511)], 0, 1, 1, 1, ref.BILINEAR)[1] == (1023, 1023)
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError):
        plan(ops, [(513, 513)], 0, 1, 1, 1, ref.BILINEAR)
    # the list form reads neither pad nor top_k
    plan(ops, [(10, 10)], 1, 3, 8, 8, ref.BICUBIC, pad=9.0, top_k=0)


def test_bad_arguments(ops):
    from ppyolo_hip import _lib
    lib = _lib.lib()
    descs = ops.pil_crop_descs([(8, 30, 10, 10)])
    ws = ctypes.c_size_t(0)
    assert lib.ppy_pil_crop_plan_bytes(1, None, 0, 4, 8, 8, 3, 0.0, 1, ctypes.byref(ws), None, None) == -1          # PPY_ERR_BAD_ARG
    assert lib.ppy_pil_crop_plan_bytes(0, descs, 0, 4, 8, 8, 3, 0.0, 1, ctypes.byref(ws), None, None) != _lib.OK
    assert lib.ppy_pil_crop_plan_bytes(1025, descs, 0, 4, 8, 8, 3, 0.0, 1, ctypes.byref(ws), None, None) != _lib.OK
    assert lib.ppy_pil_crop_plan_bytes(1, descs, 2, 4, 8, 8, 3, 0.0, 1, ctypes.byref(ws), None, None) != _lib.OK      # form
    assert lib.ppy_pil_crop_plan_bytes(1, descs, 0, 4, 8, 8, 3, 0.0, 1, None, None, None) == _lib.OK                  # outputs optional
    from ppyolo_hip._lib import PPYoloHipError
    for kw in (dict(pitch=29), dict(base=0)):                          # a short pitch, a null base
        with pytest.raises(PPYoloHipError) as e:
            plan(ops, [(10, 10)], 0, 4, 8, 8, 3, **kw)
        assert 'ppy_pil_crop_plan_bytes' in str(e.value)
    plan(ops, [(1, 10)], 0, 4, 8, 8, 3, pitch=0)                       # a one-row image may carry any pitch


def test_resizer_box_refuses_pillows_two_error_cases_on_the_host(ops):
    """device='cpu': nothing here reaches a kernel -- the boxes are known on the host and are checked there."""
    from PIL import Image
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.resize import PilResizer
    r = PilResizer(ref.BICUBIC, device='cpu')
    imgs = [ref.content(10, 12, 'random', 1), ref.content(20, 8, 'random', 2)]
    good = (0, 0, 8, 20)
    for bad, words in (((-0.5, 0, 5, 5), ('image 1', "can't be negative", '-0.5')), ((0, -1, 5, 5), ('image 1', "can't be negative", '-1.0')),
                       ((0, 0, 8.5, 5), ('image 1', "can't exceed", '8.5')), ((0, 0, 5, 20.25), ('image 1', "can't exceed", '20.25')),
                       ((3, 3, 3, 9), ('image 1', 'empty')), ((0, 0, float('nan'), 5), ('image 1', 'not finite'))):
        with pytest.raises(PPYoloHipError) as e:
            r(imgs, size=(4, 4), box=[(0, 0, 12, 10), bad])
        for w in words:
            assert w in str(e.value), str(e.value)
        if "can't" in words[1]:                                        # and Pillow refuses exactly these
            with pytest.raises(ValueError):
                Image.fromarray(imgs[1]).resize((4, 4), 3, box=bad)
    for box in ([good], (0, 0, 8, 20), [(0, 0, 8), good], 'box'):
        with pytest.raises(PPYoloHipError):
            r(imgs, size=(4, 4), box=box)
    # float32 rounding comes first, as in Pillow: 8 + 1e-9 is 8
    from ppyolo_hip.resize import check_boxes
    b = check_boxes([(10, 12), (20, 8)], [(0, 0, 12, 10), (0.1, 0, 8 + 1e-9, 20)])
    assert b.dtype == np.float32 and b[1, 2] == 8 and b[1, 0] == np.float32(0.1)
    Image.fromarray(imgs[1]).resize((4, 4), 3, box=(0.1, 0, 8 + 1e-9, 20))
