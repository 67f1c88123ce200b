"""ppy_conv2d_config_info describes every conv tile configuration id, and the description is the rule set the engine, the training
step and the library's own guards worked by when they still compared id ranges.  The expectations are written out as literals
here on purpose (not computed through ppyolo_hip.engine / train).  Host-only: built as tests/test_capi_symbols.py builds it."""
import ctypes

import pytest

FP32, BF16X3, F16X2, F16X2_SLAB, F16X2_TALL, STREAM, PATCH, WS, WS_PRE, WS_KPARITY, SMALL = range(11)      # PPY_CFG_*
OPERANDS_FP32, OPERANDS_BF16X3, OPERANDS_F16X2 = range(3)
SPLITK_NONE, SPLITK_WORKSPACE, SPLITK_IN_WORKGROUP = range(3)
PPY_OK, PPY_ERR_BAD_ARG = 0, -1


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    return _lib.lib()


def info(L, cfg):
    from ppyolo_hip._lib import ConvCfgInfo
    d = ConvCfgInfo()
    assert L.ppy_conv2d_config_info(cfg, ctypes.byref(d)) == PPY_OK, cfg
    return d


def firsts(L):
    return (L.ppy_conv2d_stream_first_config(), L.ppy_conv2d_patch_first_config(), L.ppy_conv2d_ws_first_config(),
            L.ppy_conv2d_small_first_config(), L.ppy_conv2d_num_configs())


def test_id_space_layout(L):
    s0, p0, w0, sm0, n = firsts(L)
    assert (s0, p0, w0, sm0, n) == (94, 96, 97, 113, 117)


def test_family_and_local(L):
    s0, p0, w0, sm0, n = firsts(L)
    for cfg in range(n):
        d = info(L, cfg)
        if cfg < 31:
            want = (FP32, cfg, OPERANDS_FP32)
        elif cfg < 40:
            want = (BF16X3, cfg - 31, OPERANDS_BF16X3)
        elif cfg < 67:
            want = (F16X2, cfg - 31, OPERANDS_F16X2)
        elif cfg < 85:
            want = (F16X2_SLAB, cfg - 31, OPERANDS_F16X2)
        elif cfg < 94:
            want = (F16X2_TALL, cfg - 31, OPERANDS_F16X2)
        elif cfg < p0:
            want = (STREAM, cfg - s0, OPERANDS_F16X2)
        elif cfg < w0:
            want = (PATCH, cfg - p0, OPERANDS_F16X2)
        elif cfg < sm0:
            fam = WS_PRE if cfg - w0 in (4, 5, 6) else (WS_KPARITY if cfg - w0 >= 9 else WS)
            want = (fam, cfg - w0, OPERANDS_F16X2)
        else:
            want = (SMALL, cfg - sm0, OPERANDS_F16X2)
        assert (d.family, d.local, d.operands) == want, cfg


def test_capabilities(L):
    s0, p0, w0, sm0, n = firsts(L)
    small = set(range(sm0, n))
    reads = set(range(40, 67)) | set(range(85, 94)) | {w0 + i for i in (0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14, 15)} | small
    writes = set(range(40, 67)) | set(range(85, 94)) | {w0 + i for i in range(16)} | small
    kparity = {w0 + i for i in range(9, 16)}
    stats = set(range(40, n)) - kparity - small
    twin = {w0 + 9 + i: w0 + t for i, t in enumerate((0, 1, 2, 3, 1, 2, 3))}
    for cfg in range(n):
        d = info(L, cfg)
        assert bool(d.reads_presplit) == (cfg in reads), cfg
        assert bool(d.writes_presplit) == (cfg in writes), cfg
        assert bool(d.bn_stats) == (cfg in stats), cfg
        assert d.stats_twin == twin.get(cfg, -1), cfg
        want = SPLITK_NONE if s0 <= cfg < w0 else (SPLITK_IN_WORKGROUP if cfg in small else SPLITK_WORKSPACE)
        assert d.splitk_mode == want, cfg
        assert d.reads_presplit in (0, 1) and d.writes_presplit in (0, 1) and d.bn_stats in (0, 1)
    for cfg, t in twin.items():            # "otherwise identical": the same tile, and a tile that has the statistics
        a, b = info(L, cfg), info(L, t)
        assert (a.bm, a.bn) == (b.bm, b.bn) and b.bn_stats and b.family == WS


def test_tiles(L):
    s0, p0, w0, sm0, n = firsts(L)
    assert [(info(L, c).bm, info(L, c).bn, info(L, c).stages) for c in (0, 13, 14, 30)] == [(128, 128, 2), (128, 256, 2), (64, 64, 3), (64, 64, 3)]
    for stages, first in ((2, 40), (3, 49), (4, 58), (2, 67), (3, 76)):            # nine tiles per block of f16x2 ids, the bf16x3 ones with two stages
        for i in range(9):
            a, b = info(L, 31 + i), info(L, first + i)
            assert (a.bm, a.bn, a.stages) == (b.bm, b.bn, 2) and b.stages == stages
    assert [(info(L, c).bm, info(L, c).bn, info(L, c).stages) for c in (85, 86, 87, 93)] == [(192, 128, 2), (192, 256, 2), (96, 256, 2), (96, 256, 4)]
    assert [(info(L, w0 + i).bm, info(L, w0 + i).bn, info(L, w0 + i).stages) for i in (0, 3, 6, 8, 13)] == \
        [(128, 128, 3), (64, 128, 6), (128, 64, 4), (256, 128, 3), (128, 128, 2)]
    assert [(info(L, sm0 + i).bm, info(L, sm0 + i).bn) for i in range(4)] == [(32, 32), (32, 64), (32, 32), (32, 64)]
    for cfg in range(s0, w0):
        d = info(L, cfg)
        assert (d.bm, d.bn, d.stages) == (0, 0, 0)


def test_out_of_range(L):
    from ppyolo_hip._lib import ConvCfgInfo
    d = ConvCfgInfo()
    n = L.ppy_conv2d_num_configs()
    for cfg in (-1, -7, n, n + 100):
        assert L.ppy_conv2d_config_info(cfg, ctypes.byref(d)) == PPY_ERR_BAD_ARG
    assert L.ppy_conv2d_config_info(0, None) == PPY_ERR_BAD_ARG


def test_workspace_bytes_follow_splitk_mode(L):
    n = L.ppy_conv2d_num_configs()
    for N, H, W, C, K, R, stride in ((8, 19, 19, 512, 1024, 3, 1), (1, 10, 10, 64, 256, 1, 1), (2, 33, 17, 32, 64, 3, 2), (3, 7, 9, 96, 40, 1, 1)):
        pad = (R - 1) // 2
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        chunks = R * R * (C // 32)
        for cfg in range(n):
            mode = info(L, cfg).splitk_mode
            for splitk in (1, 2, 4, 5, 64):
                s = min(splitk, chunks)
                s = -(-chunks // -(-chunks // s))            # no empty split
                got = L.ppy_conv2d_workspace_bytes(N, H, W, C, K, R, R, stride, pad, cfg, splitk)
                want = s * N * Ho * Wo * K * 4 if (mode == SPLITK_WORKSPACE and s > 1) else 0
                assert got == want, (cfg, splitk, s)


def test_python_view(L):
    from ppyolo_hip import ops
    cfgs = ops.conv_cfgs()
    assert len(cfgs) == L.ppy_conv2d_num_configs() and [d.id for d in cfgs] == list(range(len(cfgs)))
    assert ops.conv_cfg(41) is cfgs[41] and ops.conv_cfg(41) is ops.conv_cfg(41)            # read once
    for d in cfgs:
        raw = info(L, d.id)
        assert ops.CFG_FAMILIES[raw.family] == d.family and ops.CFG_OPERANDS[raw.operands] == d.operands
        assert ops.CFG_SPLITK[raw.splitk_mode] == d.splitk_mode and d.local == raw.local and d.stats_twin == raw.stats_twin
    assert (cfgs[0].family, cfgs[31].family, cfgs[40].family, cfgs[67].family, cfgs[85].family, cfgs[-1].family) == \
        ('fp32', 'bf16x3', 'f16x2', 'f16x2_slab', 'f16x2_tall', 'small')
    assert cfgs[ops.ws_first_cfg() + 4].family == 'ws_pre' and cfgs[ops.ws_first_cfg() + 9].family == 'kparity'
    from ppyolo_hip._lib import PPYoloHipError
    for bad in (-1, len(cfgs)):
        with pytest.raises(PPYoloHipError):
            ops.conv_cfg(bad)
