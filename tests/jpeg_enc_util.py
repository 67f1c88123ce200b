"""Helpers of the JPEG encoder tests that drive the C ABI: restatement dicts <-> the coefficient buffer, descriptors."""
import ctypes

import numpy as np

import jpeg_enc_ref as E

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
GUARD = 64


def params(quality=95, subsampling='4:2:0', restart_interval=0):
    from ppyolo_hip import _lib
    h, v = E.SUBSAMPLINGS.get(subsampling, (1, 1)) if isinstance(subsampling, str) else subsampling
    return _lib.JpegEncParams(quality, h, v, restart_interval)


def layout(L, p, shapes, srcs=None):
    """ppy_jpeg_enc_layout for images of the given (height, width, components) -> (rc, descs, sizes, reason)."""
    from ppyolo_hip import _lib
    n = len(shapes)
    descs = (_lib.JpegEncDesc * n)()
    for i, (h, w, c) in enumerate(shapes):
        descs[i].src, descs[i].row_stride = (srcs[i] if srcs else (0, c * w))
        descs[i].width, descs[i].height, descs[i].components = w, h, c
    sizes, reason = _lib.JpegEncSizes(), ctypes.create_string_buffer(64)
    rc = L.ppy_jpeg_enc_layout(ctypes.byref(p), n, descs, ctypes.byref(sizes), reason)
    return rc, descs, sizes, reason.value.decode()


def hd_params(hd):
    """The parameters and (height, width, components) that describe a coefficient dict (jpeg_ref / jpeg_enc_ref / jpeg_synth)."""
    c0 = hd['comps'][0]
    sub = {(1, 1): '4:4:4', (2, 1): '4:2:2', (2, 2): '4:2:0'}[(c0['h'], c0['v'])] if len(hd['comps']) == 3 else '4:4:4'
    return sub, (hd['H'], hd['W'], len(hd['comps']))


def stored(hd):
    """The image's coefficients as the seam stores them: int16, component after component, transposed inside a block."""
    return np.concatenate([np.ascontiguousarray(c['coef'].reshape(c['coef'].shape[0], c['coef'].shape[1], 8, 8).transpose(0, 1, 3, 2)).reshape(-1)
                           for c in hd['comps']]).astype(np.int16)


def natural(desc, flat):
    """The inverse of stored() for one descriptor: list of int16 [block rows, block columns, 64] in natural order."""
    out = []
    for c in range(desc.components):
        bh, bw = desc.blocks_h[c], desc.blocks_w[c]
        a = np.asarray(flat[desc.coef_offset[c]:desc.coef_offset[c] + bh * bw * 64]).reshape(bh, bw, 8, 8)
        out.append(np.ascontiguousarray(a.transpose(0, 1, 3, 2)).reshape(bh, bw, 64))
    return out


def scan_host(L, desc, coef, capacity=None):
    """ppy_jpeg_enc_scan_host with guard bytes around the output -> (rc, bytes, reason, guards intact)."""
    cap = desc.scan_capacity if capacity is None else capacity
    buf = np.full(cap + 2 * GUARD, 0xA5, np.uint8)
    used, reason = ctypes.c_size_t(0), ctypes.create_string_buffer(64)
    coef = np.ascontiguousarray(coef, np.int16)
    rc = L.ppy_jpeg_enc_scan_host(ctypes.byref(desc), coef.ctypes.data, coef.nbytes, buf.ctypes.data + GUARD, cap, ctypes.byref(used), reason)
    intact = bool((buf[:GUARD] == 0xA5).all() and (buf[GUARD + cap:] == 0xA5).all())
    return rc, buf[GUARD:GUARD + used.value].tobytes(), reason.value.decode(), intact


def header(L, p, w, h, comps, capacity=None):
    """ppy_jpeg_enc_header with guard bytes -> (rc, bytes, reason, guards intact, buffer untouched)."""
    cap = L.ppy_jpeg_enc_header_bytes(comps, p.restart_interval) if capacity is None else capacity
    buf = np.full(cap + 2 * GUARD, 0xA5, np.uint8)
    used, reason = ctypes.c_size_t(0), ctypes.create_string_buffer(64)
    rc = L.ppy_jpeg_enc_header(ctypes.byref(p), w, h, comps, buf.ctypes.data + GUARD, cap, ctypes.byref(used), reason)
    intact = bool((buf[:GUARD] == 0xA5).all() and (buf[GUARD + cap:] == 0xA5).all())
    return rc, buf[GUARD:GUARD + used.value].tobytes(), reason.value.decode(), intact, bool((buf == 0xA5).all())
