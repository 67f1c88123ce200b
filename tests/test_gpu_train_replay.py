"""Every kernel launch of a real training step (TrainStep.step: forward, loss, backward, SGD) judged on the inputs it actually
received against float64 (tests/launch_replay.py), at the sizes the step runs and with the tile / split-K choices the committed
tables make there -- the per-element check that the whole-step comparisons (test_gpu_train_step.py) cannot make through the chaos
of training-mode BatchNorm."""
import contextlib
import sys

import pytest
import torch

import launch_replay as lr
from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from ppyolo_hip import ops, synth
from ppyolo_hip.train_plan import shape_key
from test_gpu_train_step import synth_targets

pytestmark = pytest.mark.gpu


def _key_of(rec):
    return shape_key('conv', *rec['geom'])


def _prepare(cfgc, S, N, freeze_at):
    cfg = cfgc()
    cfg.backbone['freeze_at'] = freeze_at
    x = synth.synth_images(N, S, seed=11).cuda()
    gt, targets = synth_targets(cfg, N, S, 5)
    return cfg, x, gt.cuda(), [t.cuda() for t in targets]


def _choices(ts, store):
    """Record what _choose returned from a TABLE entry, by caller (forward / data gradient)."""
    real = ts._choose

    def spy(key, run, chunks, f16=False):
        tab = ts._tuned_f if f16 else ts._tuned
        hit = tab.get(key + ':f' if f16 else key)
        got = real(key, run, chunks, f16)
        if hit is not None:
            kind = 'dgrad' if _in_bwd() else 'fwd'
            store.append((kind, key, got[0], got[1]))
        return got
    ts._choose = spy


def _in_bwd():
    f = sys._getframe(2)
    while f is not None:
        if f.f_code.co_name == '_conv_unit_bwd':
            return True
        if f.f_code.co_name == 'conv_unit':
            return False
        f = f.f_back
    return False


def _step(cfg, x, gt, targets, inject=None, replay=True, monkeypatch=None):
    from ppyolo_hip.train import TrainStep
    model, _ = build_model(cfg, 0, 'cuda')
    ts = TrainStep(model, cfg)
    if inject:
        ts._tuned_f.update(inject)
    chosen = []
    _choices(ts, chosen)
    rep = lr.Replay(ops, ts)
    ctx = monkeypatch.context() if replay else contextlib.nullcontext()
    with ctx as mp:
        if replay:
            rep.install(mp)
        loss = ts.step(x, gt, targets, 0.002)
        torch.cuda.synchronize()
    return ts, rep, chosen, loss.clone(), ts.gflat.clone()


def _assert_clean(rep, title):
    print(rep.report(title))
    assert not rep.failures, rep.report(title)
    extra = set(rep.unchecked) - set(lr.ALLOWLIST)
    assert not extra, 'ops called without a replay reference: %s' % sorted(extra)
    worst = max(r['ratio'] for r in rep.census)
    assert worst <= 1.0


def _assert_covered(rep, chosen):
    """Every (key -> cfg, split-K) a table handed the step shows up as a checked launch of that geometry and id."""
    from ppyolo_hip.train import train_fwd_cfg
    by = {}
    for r in rep.census:
        if r.get('kind') in ('fwd', 'fwd-stats', 'fwd-apply', 'dgrad') and r['op'] != 'stem_conv':
            by.setdefault(('dgrad' if r['kind'] == 'dgrad' else 'fwd', _key_of(r)), []).append(r)
    missing = []
    for kind, key, c, s in chosen:
        recs = by.get((kind, key), [])
        want = (c, s) if kind == 'dgrad' else train_fwd_cfg(c, s)
        ok = any((r['cfg'], r['splitk']) == want for r in recs)
        if kind == 'fwd' and not ok:
            # the frozen C = 128 1x1 layers go to the streaming kernel whatever tile the table names (train.py: bn_epilogue_all)
            ok = ':C128:' in key and key.endswith(':R1:s1') and any(r['family'] == 'stream' and ops.conv_cfg(r['cfg']).family == 'stream'
                                                                   and r['splitk'] == 1 for r in recs)
        if not ok:
            missing.append((kind, key, c, s, [(r['cfg'], r['splitk'], r['family']) for r in recs]))
    assert not missing, missing[:10]


def _families(rep, kind):
    return {(r['family'], r['splitk']) for r in rep.census if r.get('kind') == kind}


LEGS = [
    ('r50_608_n8_fa5', PPYOLO_2x_Config, 608, 8, 5),
    ('r50_608_n8_fa3', PPYOLO_2x_Config, 608, 8, 3),
    ('r18_416_n8_fa5', PPYOLO_r18vd_Config, 416, 8, 5),
    ('r18_320_n4_fa0', PPYOLO_r18vd_Config, 320, 4, 0),
]


@pytest.mark.parametrize('name,cfgc,S,N,freeze_at', LEGS, ids=[leg[0] for leg in LEGS])
def test_train_step_launch_replay(name, cfgc, S, N, freeze_at, monkeypatch):
    cfg, x, gt, targets = _prepare(cfgc, S, N, freeze_at)
    ts, rep, chosen, loss, gflat = _step(cfg, x, gt, targets, monkeypatch=monkeypatch)
    _assert_clean(rep, name)
    print('table choices exercised (%d): %s' % (len(chosen), sorted(set((k, c, s) for k, _, c, s in chosen))))
    _assert_covered(rep, chosen)
    fwd, dg = _families(rep, 'fwd'), _families(rep, 'dgrad')
    wg = {r['family'] for r in rep.census if r.get('kind') == 'wgrad'}
    if name == 'r50_608_n8_fa5':
        assert any(s and s > 1 for _, s in fwd) and any(s and s > 1 for _, s in dg), (fwd, dg)
        assert {'wgrad-nine-tap-f16x2', 'wgrad-x3-f16x2'} <= wg, wg
    if name == 'r50_608_n8_fa3':
        assert any(f == 'kparity' for f, _ in dg), dg
        fam_of = lambda c: ops.conv_cfg(c).family if c >= 0 else None
        assert any(k == 'fwd' and fam_of(c) == 'kparity' for k, _, c, _ in chosen), 'no forward id remapped from k-parity'
        if any(k == 'dgrad' and fam_of(c) in ('ws', 'ws_pre') for k, _, c, _ in chosen):
            assert any(f == 'ws' for f, _ in dg), dg
        ops_seen = {r['op'] for r in rep.census}
        assert {'zero_insert', 'dcnv2_backward', 'dcnv2'} <= ops_seen, ops_seen
    if name == 'r18_320_n4_fa0':
        ops_seen = {r['op'] for r in rep.census}
        assert {'maxpool3x3s2_bwd', 'avgpool2x2_bwd', 'stem_conv'} <= ops_seen, ops_seen
        assert any(r['op'] == 'conv2d_wgrad' and r['geom'][3] == 3 for r in rep.census), 'no stem weight gradient'
    # the harness is transparent: the same step without the interceptor gives the same bits
    _, _, _, loss2, gflat2 = _step(cfg, x, gt, targets, replay=False)
    assert torch.equal(loss, loss2)
    if not any(r['op'] == 'dcnv2_backward' for r in rep.census):
        assert torch.equal(gflat, gflat2)
        return
    # dcnv2_backward scatters its data gradient with float atomics (csrc/dcn.hip), so the gradients of the trainable backbone
    # stages differ run to run in the last bits with or without the interceptor (measured: <= 2e-6 of each tensor's maximum);
    # the head's are computed before it and stay bit-identical
    base = ts.gflat.data_ptr()
    for k in ts.train_keys:
        o, n = (ts.G[k].data_ptr() - base) // 4, ts.G[k].numel()
        a, b = gflat[o:o + n], gflat2[o:o + n]
        if not k.startswith('backbone.'):
            assert torch.equal(a, b), k
        else:
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), k


def test_small_tile_ids_in_the_training_step(monkeypatch):
    """A table entry naming a wave-private small-output tile (conv_small.hip) for a head forward key and a data-gradient key: the
    forward maps it (train_fwd_cfg), the data gradient runs it, and the replay passes on those launches."""
    cfg, x, gt, targets = _prepare(PPYOLO_r18vd_Config, 416, 8, 5)
    # the geometries the step's head launches (a replay census of the plain step)
    _, rep0, _, _, _ = _step(cfg, x, gt, targets, monkeypatch=monkeypatch)
    dg = [_key_of(r) for r in rep0.census if r.get('kind') == 'dgrad' and r['family'] not in ('default-bf16x3', 'bf16x3', 'fp32')]
    fw = [_key_of(r) for r in rep0.census if r.get('kind') == 'fwd' and r['op'] == 'conv2d_train_fwd']
    assert dg and fw
    sm0 = ops.small_first_cfg()
    inject = {fw[-1] + ':f': [sm0 + 1, 1, 0.0], dg[0] + ':f': [sm0 + 3, 2, 0.0]}
    ts, rep, chosen, loss, _ = _step(cfg, x, gt, targets, inject=inject, monkeypatch=monkeypatch)
    _assert_clean(rep, 'small-tile injection')
    assert any(r.get('kind') == 'dgrad' and r['cfg'] == sm0 + 3 and _key_of(r) == dg[0] for r in rep.census), 'small dgrad tile not run'
    assert any(r.get('kind') == 'fwd' and _key_of(r) == fw[-1] and r['cfg'] == -1 for r in rep.census), 'small forward id not mapped'
    assert torch.isfinite(loss).all()
