"""The device entropy stage of the JPEG decoder on the GPU (csrc/jpeg_entropy.hip, JpegDecoder(entropy='device')): the
coefficient buffer against the host stage ppy_jpeg_entropy_decode, the pixels against the libjpeg-turbo goldens, damaged
streams against the host's status class.  Array equality everywhere."""
import numpy as np
import pytest
import torch

import jpeg_entropy_util as U
import jpeg_fixtures as F
import jpeg_ref as R

pytestmark = pytest.mark.gpu
OK, CORRUPT = U.OK, U.CORRUPT


@pytest.fixture(scope='module')
def L():
    return U.lib()


@pytest.fixture(scope='module')
def dec():
    from ppyolo_hip.jpeg import JpegDecoder
    return JpegDecoder(entropy='device')


def device_stage(L, files, subseq):
    """The files through ppy_jpeg_entropy_device -> (status, reason ids, link counters, coefficients per image), read back."""
    bt = U.Batch(L, files, subseq)
    plan, scan = torch.from_numpy(bt.plan).cuda(), torch.from_numpy(bt.scan).cuda()
    coef = torch.full((bt.coef_bytes // 2,), 0x5A5A, dtype=torch.int16, device='cuda')          # the call zeroes what it owns
    status = torch.full((3 * bt.n,), 77, dtype=torch.int32, device='cuda')
    ws = torch.empty(max(bt.ws_bytes, 16), dtype=torch.uint8, device='cuda')
    rc = L.ppy_jpeg_entropy_device(bt.n, bt.plan.ctypes.data, plan.data_ptr(), scan.data_ptr(), subseq, coef.data_ptr(), bt.coef_bytes,
                                   status.data_ptr(), ws.data_ptr(), bt.ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == OK, rc
    st, co, n = status.cpu().numpy(), coef.cpu().numpy(), bt.n
    return st[:n], st[n:2 * n], st[2 * n:], [bt.coefficients(co, i) for i in range(n)]


def _check_batch(L, files, subseq):
    st, rs, fixed, coefs = device_stage(L, files, subseq)
    assert not st.any() and not rs.any()
    for i, (b, c) in enumerate(zip(files, coefs)):
        rc, _, want, _ = U.host_stage(L, b)
        assert rc == OK and np.array_equal(c, want), i
    assert np.array_equal(fixed, U.twin(L, files, subseq)[2])          # the kernels repaired what their host twin repaired
    return fixed


@pytest.mark.parametrize('subseq', [U.SUBSEQ_MIN, U.SUBSEQ_DEFAULT])
def test_coefficients_of_the_fixtures_in_one_batch(L, subseq):
    _check_batch(L, [F.data(n) for n in F.names()], subseq)


@pytest.mark.parametrize('subseq', [U.SUBSEQ_MIN, U.SUBSEQ_DEFAULT])
def test_coefficients_of_synthetic_files(L, subseq):
    """A third of the CPU test's synthetic set plus its 1 x 1 and 130 x 131 files (the 1 x 1 files hold less than one
    subsequence of data) and the input of the cross-workgroup test, whose link step must have run at the smallest size."""
    cases = U.synth_cases()
    pick = [b for i, (n, b) in enumerate(cases) if i % 3 == 0 or '-1x1-' in n or '-130x131-' in n]
    assert any(len(b) - R.parse(b)['data'] - 2 < U.SUBSEQ_MIN for b in pick)
    fixed = _check_batch(L, pick + [U.link_case()], subseq)
    assert (fixed[-1] > 0) == (subseq == U.SUBSEQ_MIN)


def _same_pixels(name, t):
    got = t.cpu().numpy()
    return got.shape == F.pixels(name).shape and np.array_equal(got, F.pixels(name)) and F.matches_golden(name, got)


@pytest.mark.parametrize('name', F.names())
def test_pixels_one_by_one(dec, name):
    got = dec.imdecode(F.data(name))
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
    assert _same_pixels(name, got)


def test_pixels_mixed_batch_repeated(dec):
    """Every fixture in one call, several times, so both staging buffers come round."""
    names = F.names()
    datas = [F.data(n) for n in names]
    for _ in range(4):
        outs = dec.decode(datas)
        assert len(outs) == len(names)
        for n, t in zip(names, outs):
            assert _same_pixels(n, t), n
    assert dec.last_status.shape == (3, len(names)) and not dec.last_status[:2].any()


def test_pixels_into_strided_views(dec):
    """out= views of wider buffers, as test_gpu_jpeg.py::test_row_stride; twice, on both staging buffers."""
    names = ['c420_37x53', 'orient6_21x13', 'c444_opt_q35_50x50', 'c420_1x1']
    for _ in range(2):
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


def test_smallest_subsequences_and_orientation_off():
    from ppyolo_hip.jpeg import JpegDecoder
    raw = JpegDecoder(entropy='device', subseq_bytes=U.SUBSEQ_MIN, apply_orientation=False, threads=1)
    names = F.names()
    for n, t in zip(names, raw.decode([F.data(n) for n in names])):
        assert np.array_equal(t.cpu().numpy(), F.pixels(n, oriented=False)), n


@pytest.mark.parametrize('name,kind', F.refused())
def test_refused_files_raise(dec, name, kind):
    from ppyolo_hip._lib import PPYoloHipError
    with pytest.raises(PPYoloHipError) as e:
        dec.imdecode(F.data(name))
    assert ('progressive' in str(e.value) and 'unsupported' in str(e.value)) if kind == 'unsupported' else 'corrupt' in str(e.value)
    with pytest.raises(PPYoloHipError) as e:          # inside a batch the message names the item
        dec.decode([F.data('c420_37x53'), F.data(name)])
    assert 'item 1' in str(e.value)


def test_detect_files_equals_detect_raw(dec):
    """Decode.detect_files(files, decoder=the device-entropy decoder) == Decode.detect_raw(the golden pixels), exactly."""
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = 320
    model, _ = build_model(cfg, 0, 'cuda')
    det = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
    names = F.names()
    got = det.detect_files([F.data(n) for n in names], decoder=dec)
    want = det.detect_raw([F.pixels(n) for n in names])
    assert len(got) == len(want) == len(names)
    for n, g, w in zip(names, got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and np.array_equal(a, b), n


def _damaged_subset(L):
    """At most 64 damaged streams of the CPU sweeps, fixed by a seed: the truncated fixture, a byte flip that creates a
    marker in the middle of the entropy data, one that destroys a restart marker, and a seeded draw from the prefixes and
    byte flips.  Only streams whose header passes (the pre-pass, like ppy_jpeg_info, refuses the others before any GPU work),
    each with the status class the host stage gives it."""
    b = F.data(U.FLIP_FILE)
    start = R.parse(b)['data']
    rst = b.index(b'\xff\xd0', start)
    mid = next(i for i in range(start + (len(b) - start) // 2, len(b)) if b[i] not in (0, 0xFF) and b[i - 1] != 0xFF and b[i + 1] != 0)
    picked = [F.data('truncated_c420_37x53'), b[:mid] + b'\xff' + b[mid + 1:], b[:rst + 1] + b'\x00' + b[rst + 2:]]
    pool = [m for _, m in U.flips() if m[:start] == b[:start]]
    for name, stride in U.PREFIX_SWEEPS[:3]:
        pool += [m for m in U.prefixes(name, stride) if len(m) > R.parse(F.data(name))['data']]
    rng = np.random.default_rng(64)
    picked += [pool[i] for i in rng.choice(len(pool), 61, replace=False)]
    out = []
    for m in picked:
        rc = U.host_stage(L, m)[0]
        assert rc in (OK, CORRUPT)
        out.append((m, rc))
    return out


def test_damaged_streams(L, dec):
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.jpeg import JpegDecoder
    cases = _damaged_subset(L)
    assert len(cases) <= 64 and sum(rc == CORRUPT for _, rc in cases) >= 16 and cases[1][1] == CORRUPT and cases[2][1] == CORRUPT
    good = ['c420_37x53', 'grey_29x43']
    device_side = []
    for m, rc in cases:                      # first the host twin of the kernels, on the CPU
        pre = U.prepass(L, m)[0]
        assert U.device_stage_class(L, m, dec.subseq_bytes) == rc
        if pre == OK:
            device_side.append((m, rc))
        else:                                # found by the marker pass: raised before any GPU work, naming the item
            with pytest.raises(PPYoloHipError) as e:
                dec.decode([F.data(good[0]), m])
            assert 'item 1' in str(e.value) and 'corrupt' in str(e.value)
    assert sum(rc == CORRUPT for _, rc in device_side) >= 8
    # one by one inside a batch: the error names the item, and a good batch right after equals its goldens
    for m, rc in device_side[:12]:
        if rc == CORRUPT:
            with pytest.raises(PPYoloHipError) as e:
                dec.decode([F.data(good[0]), m, F.data(good[1])])
            assert 'item 1' in str(e.value) and 'corrupt JPEG' in str(e.value) and '(code -5)' in str(e.value)
        else:
            dec.decode([F.data(good[0]), m, F.data(good[1])])
        for n, t in zip(good, dec.decode([F.data(n) for n in good])):
            assert _same_pixels(n, t), n
    # all of them in one batch without the read-back: the status tensor carries the codes
    lazy = JpegDecoder(entropy='device')
    hb = lazy.entropy_decode([m for m, _ in device_side])
    outs = lazy.reconstruct(hb, check=False)
    assert len(outs) == len(device_side) and hb.status is lazy.last_status
    st = hb.status.cpu().numpy()
    assert st[0].tolist() == [rc for _, rc in device_side]
    assert all((r != 0) == (rc != OK) and L.ppy_jpeg_reason_string(int(r)) != b'?' for r, (_, rc) in zip(st[1], device_side))
    for n, t in zip(good, lazy.decode([F.data(n) for n in good])):
        assert _same_pixels(n, t), n
    for n, t in zip(good, dec.decode([F.data(n) for n in good])):
        assert _same_pixels(n, t), n
