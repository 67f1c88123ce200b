"""Every (cfg, split-K) a committed table can hand the training forward maps to an id that forward accepts
(ppyolo_hip/train.py:train_fwd_cfg).  Host-only: the id ranges come from the library, built as tests/test_capi_symbols.py builds it."""
import json
import os

import pytest


@pytest.fixture(scope='module')
def K():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import ops
    return ops


def _tables():
    from ppyolo_hip import train
    d = os.path.dirname(train.__file__)
    f16 = [os.path.join(d, 'tuned_gfx950_f16x2.json'), train.TRAIN_TABLE_F16]
    x3 = [os.path.join(d, 'tuned_gfx950_bf16x3.json'), train.TRAIN_TABLE]
    return [(p, True) for p in f16] + [(p, False) for p in x3]


def _accepted(K, cfg, splitk, f16):
    """The training forward's launch rules: on the f16x2 operands, statistics from the epilogue need a family that writes them
    (conv_x3.hip f16x2 tiles, conv_stream.hip, conv_patch.hip, conv_ws.hip tiles 0..8) -- the k-parity and small-output ids do
    not; on the bf16x3 operands no f16x2-only family at all."""
    if cfg == -1:
        return True
    if cfg < 0 or splitk < 1:
        return False
    ws0, sm0 = K.ws_first_cfg(), K.small_first_cfg()
    if K.stream_first_cfg() <= cfg < ws0 and splitk != 1:
        return False            # conv_igemm.hip dispatch_cfg: the streaming / patch kernels take no split-K
    if not f16:
        return cfg < K.stream_first_cfg()
    return cfg < ws0 + 9 and cfg < sm0


def test_train_fwd_cfg_maps_every_table_entry(K):
    from ppyolo_hip.train import train_fwd_cfg
    seen = 0
    for path, f16 in _tables():
        with open(path) as fh:
            tab = json.load(fh)
        for key, ent in tab.items():
            if not key.startswith('conv:'):
                continue
            c, s = train_fwd_cfg(ent[0], ent[1])
            assert _accepted(K, c, s, f16), (os.path.basename(path), key, ent, (c, s))
            seen += 1
    assert seen > 400


def test_train_fwd_cfg_rules(K):
    from ppyolo_hip.train import train_fwd_cfg
    ws0, sm0 = K.ws_first_cfg(), K.small_first_cfg()
    assert sm0 == ws0 + 16 and len(K.conv_cfgs()) == sm0 + 4
    assert train_fwd_cfg(ws0 + 9, 4) == (ws0 + 0, 4)          # k-parity 128x128 -> the same tile with one consumer group
    assert train_fwd_cfg(ws0 + 15, 1) == (ws0 + 3, 1)
    for c in range(sm0, sm0 + 4):
        for s in (1, 2, 4):
            assert train_fwd_cfg(c, s) == (-1, 0)            # a small-output tile: no statistics, k-parts not splits
    for c in (-1, 40, 66, ws0, ws0 + 8):
        assert train_fwd_cfg(c, 2) == (c, 2)


def _old_rule(K, cfg, splitk):
    """train_fwd_cfg as it stood before the library described its ids, range by range."""
    ws0 = K.ws_first_cfg()
    if ws0 + 9 <= cfg < ws0 + 16:
        return ws0 + (0, 1, 2, 3, 1, 2, 3)[cfg - ws0 - 9], splitk
    if cfg >= K.small_first_cfg():
        return -1, 0
    return cfg, splitk


def test_train_fwd_cfg_matches_the_range_rule(K):
    from ppyolo_hip.train import train_fwd_cfg
    pairs = [(c, s) for c in range(-1, len(K.conv_cfgs())) for s in (1, 2, 4)]
    for path, _ in _tables():
        with open(path) as fh:
            pairs += [(ent[0], ent[1]) for key, ent in json.load(fh).items() if key.startswith('conv:')]
    assert len(pairs) > 700
    for c, s in pairs:
        assert train_fwd_cfg(c, s) == _old_rule(K, c, s), (c, s)


def test_training_tune_candidates(K):
    from ppyolo_hip.train import tune_cfgs
    ws0 = K.ws_first_cfg()
    assert tune_cfgs(False) == list(range(31, 40))
    assert tune_cfgs(True) == list(range(40, 67)) + [ws0 + i for i in range(9)]
