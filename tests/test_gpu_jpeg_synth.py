"""The device stage of the JPEG decoder (csrc/jpeg.hip: inverse DCT, upsampling, colour, orientation, store) driven from
its seam, the int16 coefficient buffer, with seeded coefficients (tests/jpeg_synth.py) at the geometries where those
kernels can go wrong.  The expected pixels are always jpeg_ref.reconstruct of the same coefficients.  Array equality
everywhere; no Pillow, nothing outside the repository."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_ref as R
import jpeg_synth as S

pytestmark = pytest.mark.gpu


def device_reconstruct(hds, apply_orientation=True, out=None):
    """Coefficient dicts -> list of uint8 [h, w, 3] device tensors through the C ABI alone, the way JpegDecoder.reconstruct
    goes: descriptors, the packed coefficient buffer (per-image bases multiples of 16 bytes, components contiguous, a block's
    64 values stored column-major), ppy_jpeg_pack_table, one copy of [table | coefficients], ppy_jpeg_reconstruct_u8."""
    from ppyolo_hip import _lib
    L = _lib.lib()
    n = len(hds)
    descs = (_lib.JpegDesc * n)()
    base, parts = 0, []
    for d, hd in zip(descs, hds):
        d.width, d.height, d.components, d.orientation = hd['W'], hd['H'], len(hd['comps']), hd['orientation']
        off = 0
        for c, comp in enumerate(hd['comps']):
            bh, bw = comp['coef'].shape[:2]
            d.h_samp[c], d.v_samp[c], d.blocks_w[c], d.blocks_h[c], d.coef_offset[c] = comp['h'], comp['v'], bw, bh, off
            d.quant[c][:] = [int(v) for v in np.asarray(hd['q'][comp['tq']]).reshape(8, 8).T.reshape(64)]
            parts.append((base // 2 + off, comp['coef'].astype(np.int16).reshape(bh, bw, 8, 8).transpose(0, 1, 3, 2).reshape(-1)))
            off += bh * bw * 64
        d.coef_bytes, d.coef_base = off * 2, base
        base += (off * 2 + 15) // 16 * 16
    tb = L.ppy_jpeg_table_bytes(n)
    assert tb > 0 and tb % 16 == 0
    host = np.zeros(tb + base, np.uint8)
    coef = host[tb:].view(np.int16)
    for at, blocks in parts:
        coef[at:at + blocks.size] = blocks
    shapes = [(hd['W'], hd['H']) if apply_orientation and hd['orientation'] >= 5 else (hd['H'], hd['W']) for hd in hds]
    if out is None:
        out = [torch.empty((h, w, 3), dtype=torch.uint8, device='cuda') for h, w in shapes]
    assert [tuple(t.shape) for t in out] == [(h, w, 3) for h, w in shapes] and all(t.stride(1) == 3 and t.stride(2) == 1 for t in out)
    ws_bytes = L.ppy_jpeg_workspace_bytes(n, descs)
    assert ws_bytes == sum(comp['coef'].size for hd in hds for comp in hd['comps'])          # one byte per block-padded sample
    assert L.ppy_jpeg_pack_table(n, descs, (ctypes.c_void_p * n)(*[t.data_ptr() for t in out]),
                                 (ctypes.c_longlong * n)(*[max(t.stride(0), 3 * t.shape[1]) for t in out]), int(apply_orientation),
                                 host.ctypes.data, tb) == 0
    blob = torch.from_numpy(host).cuda()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    rc = L.ppy_jpeg_reconstruct_u8(n, descs, int(apply_orientation), blob.data_ptr(), blob.data_ptr() + tb, base, ws.data_ptr(), ws_bytes,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ppy_error_string(rc)
    torch.cuda.synchronize()
    return out


def check(hds, apply_orientation=True, batch=64):
    for i in range(0, len(hds), batch):
        part = hds[i:i + batch]
        for k, (hd, t) in enumerate(zip(part, device_reconstruct(part, apply_orientation))):
            want = R.reconstruct(hd, apply_orientation)
            got = t.cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), \
                (i + k, hd['W'], hd['H'], hd['orientation'], [(c['h'], c['v']) for c in hd['comps']], int((got != want).sum()))


# ------------------------------------------------------------------------------------------------------- the geometry sweep
SIDES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 255, 256, 257, 258, 259, 513]
SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]
GROUPS = 4


def size_pairs():
    """(H, W): every side once as the width and once as the height, a large side always beside a small one."""
    out = []
    for i, s in enumerate(SIDES):
        out += [(SMALL[i % len(SMALL)], s), (s, SMALL[(3 * i + 1) % len(SMALL)])]
    return out + [(31, 33), (33, 31), (17, 15), (16, 16)]


def sweep_specs(group=None):
    """(sampling, orientation, H, W) for every sampling x orientation x size pair; the samplings alternate, so every batch
    of 64 mixes samplings, orientations and sizes.  group: one of GROUPS slices of the size pairs."""
    pairs = size_pairs()
    if group is not None:
        pairs = pairs[group::GROUPS]
    return [(s, o, h, w) for h, w in pairs for o in range(1, 9) for s in S.SAMPLINGS]


def test_sweep_reaches_the_wide_cases():
    specs = sweep_specs()
    assert sorted(set(sum(([h, w] for _, _, h, w in specs), []))) == SIDES
    assert sum(len(sweep_specs(g)) for g in range(GROUPS)) == len(specs) == len(size_pairs()) * 32
    for sampling in ('422', '420'):
        assert any(s == sampling and o == 1 and w > 256 for s, o, h, w in specs)                 # blockIdx.x > 0, stored raster
        assert any(s == sampling and o >= 5 and h > 256 for s, o, h, w in specs)                 # output width = stored height
        assert any(s == sampling and o == 1 and h > 256 for s, o, h, w in specs)                 # blockIdx.y > 0
        assert any(s == sampling and -(-w // 2) <= 2 for s, o, h, w in specs)                    # the box fallback
        assert any(s == sampling and w > 2 and w % 2 == 1 for s, o, h, w in specs)               # the dw - 1 edge tap
    assert any(s == '420' and h % 2 == 1 and h > 2 for s, o, h, w in specs)                      # the dh - 1 edge tap
    assert all(h * w <= 513 * 17 for _, _, h, w in specs)


@pytest.mark.parametrize('group', range(GROUPS))
@pytest.mark.parametrize('regime', ['natural', 'zone_b'])
def test_geometry_sweep(regime, group):
    rng = np.random.default_rng(100 + group)
    check([S.synth(rng, h, w, s, regime, orientation=o) for s, o, h, w in sweep_specs(group)])


def test_orientation_off():
    rng = np.random.default_rng(104)
    check([S.synth(rng, h, w, s, 'natural', orientation=o) for s, o, h, w in sweep_specs(0)[::3]], apply_orientation=False)


# --------------------------------------------------------------------------------------------------------- block regimes
def segments(hd):
    """Share of the inverse-DCT samples in each of the four segments of the range-limit table (ramp up, 255, 0, ramp)."""
    x = np.concatenate([R.plane(c, hd['q'], prelimit=True).ravel() for c in hd['comps']]) & 1023
    return [float(((x >= a) & (x < b)).mean()) for a, b in ((0, 128), (128, 512), (512, 896), (896, 1024))]


@pytest.mark.parametrize('sampling', ['grey', '444'])
@pytest.mark.parametrize('regime', ['dc_only', 'one_ac', 'zone_b', 'zone_c'])
def test_block_regimes(regime, sampling):
    """A few hundred blocks per component; zone_c over the whole int16 x uint16 range, which only the seam can carry."""
    rng = np.random.default_rng(200)
    hd = S.synth(rng, 96, 200, sampling, regime, legal=False)
    for c in hd['comps']:
        co = c['coef'].reshape(-1, 64)
        if regime == 'one_ac':
            assert set(np.nonzero(co[:, 1:])[1] + 1) == set(range(1, 64))
        if regime == 'dc_only':
            assert not co[:, 1:].any() and co[:, 0].any()
        if regime == 'zone_c':
            a, b = R.plane(c, hd['q']), R.plane(c, hd['q'], wide=True)
            d = (a != b).reshape(a.shape[0] // 8, 8, a.shape[1] // 8, 8).any((1, 3))
            assert d.mean() >= 0.9, d.mean()
            assert np.abs(co.astype(np.int64)).max() > 30000 and hd['q'][c['tq']].max() > 60000
    if regime == 'zone_b':
        seg = segments(hd)
        print('zone_b samples per segment of the range-limit table:', seg)
        assert min(seg) >= 0.05, seg
    check([hd])


# ---------------------------------------------------------------------------------------------------- COCO-sized batch
COCO = [(480, 640, '420', 1), (480, 640, '420', 6), (375, 500, '422', 1), (427, 640, 'grey', 1), (500, 333, '444', 1),
        (640, 427, '420', 8), (612, 612, '422', 3), (360, 640, '420', 5)]          # (H, W, sampling, orientation)


@pytest.fixture(scope='module')
def coco():
    rng = np.random.default_rng(300)
    hds = [S.synth(rng, h, w, s, 'natural', orientation=o) for h, w, s, o in COCO]
    want = [R.reconstruct(hd) for hd in hds]
    for w in want:
        w.setflags(write=False)
    return hds, want


def test_coco_batch_from_coefficients(coco):
    hds, want = coco
    outs = device_reconstruct(hds)
    for i, (t, w) in enumerate(zip(outs, want)):
        assert tuple(t.shape) == w.shape and np.array_equal(t.cpu().numpy(), w), COCO[i]


@pytest.mark.parametrize('dri', [0, 5])
@pytest.mark.parametrize('tables', ['flat', 'skewed'])
def test_coco_batch_as_files(coco, tables, dri):
    """End to end: the library's own host stage on files written from the same coefficients."""
    from ppyolo_hip.jpeg import JpegDecoder
    hds, want = coco
    outs = JpegDecoder().decode([S.encode(hd, dri, tables) for hd in hds])
    for i, (t, w) in enumerate(zip(outs, want)):
        assert tuple(t.shape) == w.shape and np.array_equal(t.cpu().numpy(), w), COCO[i]


# ---------------------------------------------------------------------------------------------------- grids and strides
def test_grid_sized_by_three_images():
    """A 1 x 1025 image, a 1025 x 1 image, a 64 x 64 4:2:0 image (96 blocks, fewer than either) and one of more blocks than
    all: the widest, the tallest and the image of most blocks are three different entries, in either order of the batch."""
    rng = np.random.default_rng(400)
    hds = [S.synth(rng, 1, 1025, 'grey', 'natural'), S.synth(rng, 1025, 1, '444', 'natural'), S.synth(rng, 64, 64, '420', 'natural'),
           S.synth(rng, 136, 136, '420', 'natural', orientation=6)]
    blocks = [sum(c['coef'].shape[0] * c['coef'].shape[1] for c in hd['comps']) for hd in hds]
    # 129, 387, 96 and 486 blocks: width, height and block count are each the largest in a different entry
    assert (int(np.argmax([hd['W'] for hd in hds])), int(np.argmax([hd['H'] for hd in hds])), int(np.argmax(blocks))) == (0, 1, 3)
    check(hds)
    check(hds[::-1])


def test_strided_outputs():
    """Subsampled images, widths over 256 included, decoded into views at column offset 1-3 of wider buffers: rows that are
    not 4-byte aligned take the byte-store path, and nothing outside the view is written."""
    rng = np.random.default_rng(500)
    specs = [sp for sp in sweep_specs() if sp[0] in ('422', '420')][5::7]
    assert any(w > 256 and o == 1 for _, o, h, w in specs) and any(h > 256 and o >= 5 for _, o, h, w in specs)
    hds = [S.synth(rng, h, w, s, 'natural', orientation=o) for s, o, h, w in specs]
    for i in range(0, len(hds), 64):
        part = hds[i:i + 64]
        wide, outs, offs = [], [], []
        for k, hd in enumerate(part):
            oh, ow = (hd['W'], hd['H']) if hd['orientation'] >= 5 else (hd['H'], hd['W'])
            off = 1 + k % 3
            big = torch.full((oh, ow + off + k % 4, 3), 0xA5, dtype=torch.uint8, device='cuda')
            wide.append(big)
            offs.append(off)
            outs.append(big[:, off:off + ow])
        res = device_reconstruct(part, out=outs)
        assert all(a is b for a, b in zip(res, outs))
        for hd, big, off in zip(part, wide, offs):
            want = R.reconstruct(hd)
            got = big.cpu().numpy()
            assert np.array_equal(got[:, off:off + want.shape[1]], want), (hd['W'], hd['H'], hd['orientation'])
            assert np.all(got[:, :off] == 0xA5) and np.all(got[:, off + want.shape[1]:] == 0xA5), (hd['W'], hd['H'], hd['orientation'])
