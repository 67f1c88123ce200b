"""What the training step decides without a device (ppyolo_hip/train_plan.py), checked on the CPU: table keys, the forward form of a
convolution unit, the flat parameter layout and its all-reduce buckets, the detection block's schedule, the switches.  Tile
descriptors are a small table, as in tests/test_plan_host_logic.py; tests/test_train_cfg_ids.py checks the id rules on the library's."""
import collections
import json
import re

import pytest

from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from ppyolo_hip import train_plan as TP

CONFIGS = [('r50vd', PPYOLO_2x_Config), ('r18vd', PPYOLO_r18vd_Config)]


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
KEY = re.compile(r'^(conv|dcnf):N(\d+):H(\d+):W(\d+):C(\d+):K(\d+):R(\d+):s(\d+)(:f)?(:p)?(:g)?$')


def test_every_training_table_key_formats_back():
    from ppyolo_hip import train
    seen = 0
    for path in (train.TRAIN_TABLE, train.TRAIN_TABLE_F16):
        with open(path) as fh:
            tab = json.load(fh)
        for key in tab:
            m = KEY.match(key)
            assert m, key
            g = m.groups()
            assert TP.shape_key(g[0], *[int(v) for v in g[1:8]], f=bool(g[8]), p=bool(g[9]), g=bool(g[10])) == key
            seen += 1
    assert seen > 50


def test_tune_key_is_the_formatter():
    from ppyolo_hip.plan_links import tune_key
    X = collections.namedtuple('X', 'N H W')
    W = collections.namedtuple('W', 'shape')
    for kind, name in (('conv', 'conv'), ('dcn', 'dcnf')):
        for f in (False, True):
            for p in (False, True):
                for g in (False, True):
                    op = dict(op=kind, x=X(8, 76, 38), w=W((256, 3, 3, 128)), stride=2, wf16=1 if f else None, amax_in_id=0 if f else None,
                              pool=object() if p else None, gp_in=g)
                    want = '%s:N8:H76:W38:C128:K256:R3:s2%s%s%s' % (name, ':f' if f else '', ':p' if p else '', ':g' if g else '')
                    assert tune_key(op) == want == TP.shape_key(name, 8, 76, 38, 128, 256, 3, 2, f, p, g)
                    assert tune_key(op, False) == TP.shape_key(name, 8, 76, 38, 128, 256, 3, 2, f, p)


def test_dgrad_key_is_the_transposed_geometry():
    assert TP.dgrad_key(8, 19, 19, 27, 2048, 3) == ('conv:N8:H19:W19:C32:K2048:R3:s1', 9)         # K = 27 (conv_offset): C' = 32
    assert TP.dgrad_key(2, 38, 38, 512, 288, 1) == ('conv:N2:H38:W38:C512:K288:R1:s1', 16)


# ---- the forward form ---------------------------------------------------------------------------------------------------------------
Cfg = collections.namedtuple('Cfg', 'id family local splitk_mode bn_stats stats_twin')
TILES = [Cfg(0, 'f16x2', 0, 'workspace', True, -1), Cfg(1, 'bf16x3', 0, 'workspace', False, -1), Cfg(2, 'stream', 0, 'none', True, -1),
         Cfg(3, 'stream', 1, 'none', True, -1), Cfg(4, 'kparity', 0, 'workspace', False, 0), Cfg(5, 'small', 0, 'workgroup', False, -1)]
STREAM0 = 2


def _sw(**kw):
    return TP.switches({}, 1, False, False)._replace(**kw)


def _form(table, sw=None, has_bn=True, f16=True, trainable=False, coord=False, R=1, S=1, stride=1, C=128, Kout=512, HW=76 * 76):
    return TP.conv_form(has_bn, f16, trainable, coord, R, S, stride, C, Kout, HW, table, sw or _sw(), TILES.__getitem__, STREAM0)


def test_forward_form_of_the_frozen_c128_layers():
    assert _form((0, 1)) == ('epilogue', STREAM0, 1) == _form((0, 4)) == _form((-1, 0))       # whatever the table names
    assert _form((3, 1)) == ('epilogue', 3, 1)                                                 # the table's own streaming variant
    one = _sw(bn_epilogue_all=False)                                                           # PPYOLO_HIP_TRAIN_BN_EPILOGUE=1
    for kw in (dict(Kout=384), dict(HW=16), dict(trainable=True), dict(coord=True), dict(sw=one)):
        assert _form((0, 1), **kw) == ('stats', 0, 1), kw
        assert _form((0, 2), **kw) == ('plain', 0, 2), kw
    # ... unless the table names the streaming kernel (which the shape conditions do not bind)
    for kw in (dict(Kout=384), dict(HW=16), dict(sw=one), dict(C=256)):
        assert _form((3, 1), **kw) == ('epilogue', 3, 1), kw
    for kw in (dict(trainable=True), dict(coord=True), dict(sw=_sw(bn_epilogue=False, bn_epilogue_all=False)), dict(sw=_sw(fuse_stats=False))):
        assert _form((3, 1), **kw)[0] != 'epilogue', kw
    assert _form((0, 1), R=3, S=3) == ('stats', 0, 1) and _form((0, 1), stride=2) == ('stats', 0, 1)
    assert _form((0, 1), C=256) == ('stats', 0, 1) and _form((0, 1), Kout=128 * 32) == ('stats', 0, 1)


def test_forward_form_statistics_from_the_epilogue():
    kw = dict(C=256, R=3, S=3)
    assert _form((0, 1), **kw) == ('stats', 0, 1)
    assert _form((0, 2), **kw) == ('plain', 0, 2)                     # partial sums in memory: no statistics in the epilogue
    assert _form((1, 1), **kw) == ('plain', 1, 1)                     # a tile that writes none
    assert _form((-1, 0), **kw) == ('plain', -1, 0)
    assert _form((0, 1), f16=False, **kw) == ('plain', 0, 1)
    assert _form((0, 1), sw=_sw(fuse_stats=False), **kw) == ('plain', 0, 1)
    assert _form((4, 2), **kw) == ('plain', 0, 2) and _form((4, 1), **kw) == ('stats', 0, 1)      # k-parity -> its twin (train_fwd_cfg)
    assert _form((5, 2), **kw) == ('plain', -1, 0)


def test_forward_form_without_batchnorm_and_in_fp32():
    for table in ((0, 1), (3, 1), (-1, 0), (0, 2)):
        for kw in (dict(), dict(C=256, R=3, S=3), dict(coord=True)):
            assert _form(table, has_bn=False, **kw)[0] == 'plain'
            assert _form(table, sw=_sw(fp32=True, f16=False), f16=False, **kw) == ('plain', -1, 0)


# ---- layout and buckets -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def models():
    return {name: build_model(cfgc(), 0, 'cpu')[0] for name, cfgc in CONFIGS}


@pytest.mark.parametrize('freeze_at', [5, 3, 0])
@pytest.mark.parametrize('name', [c[0] for c in CONFIGS])
def test_flat_layout_and_buckets(models, name, freeze_at):
    params = [(k, tuple(p.shape)) for k, p in models[name].named_parameters() if TP.stage_of(k) > freeze_at]
    keys = [k for k, _ in params]
    assert keys and (freeze_at < 5) == any(k.startswith('backbone.') for k in keys)
    shapes = [(k, TP.kernel_shape(s)) for k, s in params]
    for (k, s), (_, ks) in zip(params, shapes):
        if len(s) == 4:
            assert ks == (s[0], s[2], s[3], (s[1] + 31) // 32 * 32), k           # KRSC, input channels padded to 32
        else:
            assert ks == s
    layout, total, n_decay = TP.flat_layout(shapes)
    assert list(layout) != keys and sorted(layout) == sorted(keys)
    spans = sorted((o, o + n, k) for k, (o, n, _) in layout.items())
    for k, (o, n, shp) in layout.items():
        assert o % 64 == 0 and shp == dict(shapes)[k]
        cnt = 1
        for d in shp:
            cnt *= d
        assert n == cnt
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total and total % 64 == 0
    decays = {k for k, s in params if len(s) == 4 or k.endswith('.conv_offset.bias')}
    assert {k for a, e, k in spans if e <= n_decay} == decays and all(a >= n_decay for a, e, k in spans if k not in decays)
    assert 0 < n_decay < total and n_decay % 64 == 0
    bk = TP.buckets(keys, layout, total)
    ranges = sorted((a, e, b) for b, v in bk.items() for a, e in v['ranges'])
    assert ranges[0][0] == 0 and ranges[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))           # disjoint, and their union is [0, total)
    for k, (o, n, _) in layout.items():
        b = TP.bucket_of(k)
        assert any(a <= o and o + n <= e for a, e in bk[b]['ranges']), k
        assert TP.unit_of(k) in bk[b]['units']
    assert set(bk) == {TP.bucket_of(k) for k in keys}
    if freeze_at == 3:
        assert {'stage4', 'stage5', 'head.tail', 'head.detection_blocks.0'} <= set(bk) and 'stage3' not in bk


# ---- the detection block's schedule -----------------------------------------------------------------------------------------------------
def _variants(cfgc):
    base = cfgc().head
    out = [{}]
    for k in ('spp', 'drop_block', 'coord_conv'):
        out.append({k: not base[k]})
    return out + [dict(conv_block_num=1)]


@pytest.mark.parametrize('name,cfgc,change', [(n, c, v) for n, c in CONFIGS for v in _variants(c)],
                         ids=['%s-%s' % (n, '_'.join('%s=%s' % kv for kv in v.items()) or 'configured') for n, c in CONFIGS for v in _variants(c)])
def test_detection_schedule_names_the_models_layers(name, cfgc, change):
    cfg = cfgc()
    cfg.head.update(change)
    model, _ = build_model(cfg, 0, 'cpu')
    sd = model.state_dict()
    got = {}
    for i, blk in enumerate(model.head.detection_blocks):
        p = 'head.detection_blocks.%d.layers.' % i
        want = sorted(int(k[len(p):].split('.')[0]) for k in sd if k.startswith(p) and k.endswith('.conv.weight'))
        for active in (True, False):
            steps = TP.detection_schedule(dict(cfg.head, drop_active=active), i == 0)
            convs = [s.n for s in steps if s.kind in ('conv', 'route')]
            assert convs == want, (i, convs, want)
            kinds = {j: type(m).__name__ for j, m in enumerate(blk.layers)}
            assert [s.n for s in steps if s.kind == 'drop'] == [j for j, t in kinds.items() if t == 'DropBlock']
            assert [s.n for s in steps if s.kind == 'spp'] == [j for j, t in kinds.items() if t == 'SPP']
            assert [s.kind for s in steps[-2:]] == ['route', 'tip'] and steps[-1].n == 1 and steps[-2].n == len(blk.layers) - 1
            coord = bool(cfg.head['coord_conv'])
            for s in steps:
                if s.kind in ('conv', 'route'):       # behind a CoordConv module exactly where the schedule says so
                    assert s.coord == (coord and type(blk.layers[s.n - 1]).__name__ == 'CoordConv'), (i, s)
            assert steps[-1].coord == coord
            # a tensor goes to a coordinate-ready buffer iff the next step that runs is a convolution behind a CoordConv
            run = [s for s in steps if not (s.kind == 'drop' and not active)]
            for s, nxt in zip(run, run[1:]):
                if s.kind != 'spp' and s.dest != 'spp':
                    assert (s.dest == 'coord') == (nxt.coord and nxt.kind != 'drop'), (i, s, nxt)
        got[i] = want
    if not change:
        assert got == ({0: [1, 2, 4, 6, 7, 10], 1: [1, 2, 5, 6, 8], 2: [1, 2, 5, 6, 8]} if name == 'r50vd' else {0: [2], 1: [1]})


# ---- the switches ---------------------------------------------------------------------------------------------------------------------
def test_switch_rules():
    ov = 'PPYOLO_HIP_TRAIN_OVERLAP'
    assert not TP.switches({}, 2, True, False).overlap and TP.switches({ov: '1'}, 2, True, False).overlap             # nccl: opt-in
    assert not TP.switches({ov: '0'}, 2, True, False).overlap
    assert TP.switches({}, 2, False, False).overlap and not TP.switches({ov: '0'}, 2, False, False).overlap             # gloo: on unless =0
    assert TP.switches({ov: '1'}, 2, False, False).overlap
    assert TP.switches({}, 1, True, False).overlap                    # one rank: no collective, the default
    for env in ({}, {ov: '1'}, {ov: '0'}):
        for nccl in (False, True):
            assert not TP.switches(env, 2, nccl, True).overlap        # external optimizer: always off
    for ws in ('0', '1'):
        for tail in (None, '0', '1'):
            env = {'PPYOLO_HIP_TRAIN_WGRAD_STREAM': ws}
            if tail is not None:
                env['PPYOLO_HIP_TRAIN_ASYNC_TAIL'] = tail
            s = TP.switches(env, 1, False, False)
            assert s.wgrad_side == (ws == '1') and s.async_tail == (ws == '1' and tail != '0')
    math = {m: TP.switches({'PPYOLO_HIP_TRAIN_MATH': m}, 1, False, False) for m in ('f16x2', 'bf16x3', 'fp32')}
    assert [(s.f16, s.fp32) for s in math.values()] == [(True, False), (False, False), (False, True)]
    d = TP.switches({}, 1, False, False)
    assert d == (True, True, True, True, True, False, True, True, True)
    e = {'PPYOLO_HIP_TRAIN_BN_EPILOGUE': '1'}
    assert TP.switches(e, 1, False, False)[2:4] == (True, False) and TP.switches({'PPYOLO_HIP_TRAIN_BN_EPILOGUE': '0'}, 1, False, False)[2:4] == (False, False)
    off = TP.switches({'PPYOLO_HIP_TRAIN_FUSE_STATS': '0', 'PPYOLO_HIP_TRAIN_PREFETCH': '0'}, 1, False, False)
    assert not off.fuse_stats and not off.prefetch
