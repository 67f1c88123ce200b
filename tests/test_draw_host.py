"""ppyolo_hip.draw without a GPU: the colour tables against the reference's lines, every refusal by name, the binding."""
import ctypes
import random

import numpy as np
import pytest
import torch

import draw_ref
from ppyolo_hip import _lib, label_font
from ppyolo_hip._lib import PPYoloHipError
from ppyolo_hip.draw import BoxDrawer, class_colors, label_codes


@pytest.mark.parametrize('n', [80, 20, 1, 12])
def test_colours_are_the_references(n):
    state = random.getstate()
    ref = draw_ref.reference_colors(n)          # random.seed(0); shuffle; random.seed(None), as the reference writes it
    random.setstate(state)
    assert class_colors(n) == ref
    assert BoxDrawer(['c%d' % i for i in range(n)]).colors == ref
    assert all(isinstance(c, tuple) and len(c) == 3 for c in ref)


def test_constructing_a_drawer_leaves_the_global_generator_alone():
    random.seed(1234)
    state = random.getstate()
    BoxDrawer(['a', 'b', 'c'])
    assert random.getstate() == state


def test_names_become_printable_codes():
    assert label_codes('dog') == [100, 111, 103]
    assert label_codes('caf\xe9\n') == [99, 97, 102, 63, 63]
    with pytest.raises(PPYoloHipError, match='65 characters'):
        BoxDrawer(['x' * 65])
    BoxDrawer(['x' * 64])
    with pytest.raises(PPYoloHipError, match='at least one class'):
        BoxDrawer([])


def _ok_rows(n=1, k=3, device='cpu'):
    return torch.zeros((n, k, 6), dtype=torch.float32, device=device), torch.zeros((n,), dtype=torch.int32, device=device)


def test_images_are_refused_by_name():
    d = BoxDrawer(['a', 'b'])                    # device 'cuda': nothing below reaches it
    dets, count = _ok_rows()
    good = torch.zeros((8, 9, 3), dtype=torch.uint8)
    with pytest.raises(PPYoloHipError, match='lives on cpu'):
        d([good], dets, count)
    with pytest.raises(PPYoloHipError, match='does not copy a host array'):
        d([np.zeros((8, 9, 3), np.uint8)], dets, count)
    ro = np.zeros((8, 9, 3), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(PPYoloHipError, match='does not copy a host array'):
        d([ro], dets, count)
    with pytest.raises(PPYoloHipError, match='dtype torch.float32'):
        d([good.float()], dets, count)
    with pytest.raises(PPYoloHipError, match=r'shape \(8, 9\)'):
        d([good[:, :, 0]], dets, count)
    with pytest.raises(PPYoloHipError, match=r'shape \(8, 9, 4\)'):
        d([torch.zeros((8, 9, 4), dtype=torch.uint8)], dets, count)
    with pytest.raises(PPYoloHipError, match='strides'):
        d([torch.zeros((3, 8, 9), dtype=torch.uint8).permute(1, 2, 0)], dets, count)          # CHW storage
    with pytest.raises(PPYoloHipError, match='strides'):
        d([torch.zeros((8, 18, 3), dtype=torch.uint8)[:, ::2]], dets, count)                   # pixel stride 6
    with pytest.raises(PPYoloHipError, match='empty batch'):
        d([], dets, count)


def test_rows_are_refused_by_name():
    d = BoxDrawer(['a', 'b'], device='cpu')      # lets host tensors pass the device rule; every case raises before a launch
    im = [torch.zeros((8, 9, 3), dtype=torch.uint8)]
    dets, count = _ok_rows()
    with pytest.raises(PPYoloHipError, match='dets: dtype torch.float64'):
        d(im, dets.double(), count)
    with pytest.raises(PPYoloHipError, match='count: dtype torch.int64'):
        d(im, dets, count.long())
    with pytest.raises(PPYoloHipError, match=r'expected \[1, K, 6\]'):
        d(im, dets[0], count)
    with pytest.raises(PPYoloHipError, match=r'expected \[1, K, 6\]'):
        d(im, torch.zeros((1, 3, 5)), count)
    with pytest.raises(PPYoloHipError, match=r'expected \[1, K, 6\]'):
        d(im, dets, torch.zeros((2,), dtype=torch.int32))
    with pytest.raises(PPYoloHipError, match='1025 rows'):
        d(im, torch.zeros((1, 1025, 6)), count)
    with pytest.raises(PPYoloHipError, match='contiguous'):
        d(im, torch.zeros((1, 3, 12))[:, :, ::2], count)
    with pytest.raises(PPYoloHipError, match='dets: expected a device tensor'):
        d(im, dets.numpy(), count)
    d2 = BoxDrawer(['a'])
    with pytest.raises(PPYoloHipError, match='lives on cpu'):
        d2(im, dets, count)


def test_draw_host_refusals_and_the_empty_set():
    d = BoxDrawer(['a', 'b'])
    image = np.arange(8 * 9 * 3, dtype=np.uint8).reshape(8, 9, 3)
    before = image.copy()
    assert d.draw_host(image, np.array([]), np.array([]), np.array([])) is image          # the reference's empty arrays
    assert d.draw_host(image, np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)) is image
    assert np.array_equal(image, before)
    box, cls = np.array([[1, 2, 5, 6]], np.float32), np.array([1], np.int32)
    for bad in (1.5, -0.01, np.nan, np.inf):
        with pytest.raises(PPYoloHipError, match=r'score outside \[0, 1\]'):
            d.draw_host(image, box, np.array([bad], np.float32), cls)
    with pytest.raises(PPYoloHipError, match='class outside 0..1'):
        d.draw_host(image, box, np.array([0.5], np.float32), np.array([2]))
    with pytest.raises(PPYoloHipError, match='class outside 0..1'):
        d.draw_host(image, box, np.array([0.5], np.float32), np.array([-1]))
    with pytest.raises(PPYoloHipError, match='not finite'):
        d.draw_host(image, np.array([[1, np.nan, 5, 6]], np.float32), np.array([0.5], np.float32), cls)
    with pytest.raises(PPYoloHipError, match='2 boxes, 1 scores'):
        d.draw_host(image, np.zeros((2, 4), np.float32), np.array([0.5], np.float32), cls)
    ro = image.copy()
    ro.flags.writeable = False
    with pytest.raises(PPYoloHipError, match='read-only'):
        d.draw_host(ro, box, np.array([0.5], np.float32), cls)
    with pytest.raises(PPYoloHipError, match='expected a numpy uint8 image'):
        d.draw_host(torch.zeros((8, 9, 3), dtype=torch.uint8), box, np.array([0.5], np.float32), cls)
    with pytest.raises(PPYoloHipError, match='dtype float32'):
        d.draw_host(image.astype(np.float32), box, np.array([0.5], np.float32), cls)
    with pytest.raises(PPYoloHipError, match=r'shape \(8, 9\)'):
        d.draw_host(image[:, :, 0], box, np.array([0.5], np.float32), cls)
    assert np.array_equal(image, before)


def test_c_abi_refuses_on_the_host():
    """Argument checks of ppy_draw_detections_u8 come before any device call: they run without a GPU."""
    import __graft_entry__ as ge
    ge.build()
    L = _lib.lib()
    descs = (_lib.DrawImage * 1)()
    descs[0].base, descs[0].pitch, descs[0].h, descs[0].w = 4096, 27, 8, 9
    lens = (ctypes.c_int * 2)(3, 64)
    p = 4096          # never dereferenced: every call below is refused

    def call(n=1, h_images=descs, K=100, C=2, h_len=lens, images=p, dets=p):
        return L.ppy_draw_detections_u8(n, h_images, images, dets, p, K, 0.0, p, C, p, p, h_len, p, None)

    assert call(K=0) == call(K=1025) == call(C=0) == _lib.ERR_UNSUPPORTED
    assert call(h_len=(ctypes.c_int * 2)(3, 65)) == _lib.ERR_UNSUPPORTED
    assert call(h_len=(ctypes.c_int * 2)(-1, 3)) == -1
    assert call(n=0) == call(n=65536) == call(images=None) == call(dets=None) == -1
    for field, value in (('base', None), ('h', 0), ('w', 0), ('w', 65536), ('pitch', 26)):
        bad = (_lib.DrawImage * 1)()
        ctypes.memmove(bad, descs, ctypes.sizeof(descs))
        setattr(bad[0], field, value)
        assert call(h_images=bad) == -1, field


def test_device_table_layout():
    t = label_font.device_table()
    (x0, y0, x1, y1), bits = label_font.glyph(ord('A'))
    rec = t[16 * (ord('A') - 32):16 * (ord('A') - 31)]
    assert (rec[0], rec[1], rec[2], rec[3], rec[4]) == (x0 + 1, y0, x1 + 1, y1, 0)
    assert all(rec[5 + y] == (bits[y - y0] << (x0 + 1) if y0 <= y < y1 else 0) for y in range(11))
    assert max(max(t[16 * i + 5:16 * i + 16]) for i in range(95)) < 128
