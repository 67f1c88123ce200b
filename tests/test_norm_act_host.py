"""GroupNorm / AffineChannel / Mish of Conv2dUnit without a device: the torch restatement against the reference's float32 outputs,
the units' surface (state_dict keys, optimizer groups), the plans such models record, and the training step's refusal.
The golden (tests/golden/g23_norm_act*.npz, tools/make_goldens.py --only g23) holds inputs, parameters, the reference's float32
output and its float64 output (as the float32 difference d64 to the float32 one)."""
import json
import os

import pytest
import torch

import norm_act_plans as P
import norm_act_ref as R
from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from norm_act_interp import NormActPlanRunner
from ppyolo_hip import synth
from ppyolo_hip._lib import PPYoloHipError
from ppyolo_hip.engine import Builder
from ppyolo_hip.runtime import build_plan

UNITS = R.unit_cases()


def _cfg(cfgc, backbone, head):
    cfg = cfgc()
    cfg.backbone['norm_type'], cfg.head['norm_type'] = backbone, head
    return cfg


# ---- (a) the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', UNITS, ids=[c[0] + (c[1]['special'] or '%s_%s' % (c[1]['norm'], c[1]['act'])) for c in UNITS])
def test_restatement_equals_the_reference_bit_for_bit(case):
    """F.conv2d + F.group_norm / F.batch_norm / the reference's AffineChannel arithmetic + the activations are the very ATen calls
    the reference's modules make, so float32 agrees bit for bit -- and the float64 evaluation agrees with the stored one."""
    p, meta, x, sd = case
    d = R.load()
    with torch.no_grad():
        assert torch.equal(R.unit(meta, sd, x), R.y32(d, p))
        y64 = R.unit(meta, sd, x.double())
    # (d64 is stored in float32: the reconstruction is exact to 6e-8 of the DIFFERENCE, far below one float32 ulp of y)
    assert (y64 - R.y64(d, p)).abs().max().item() <= 1e-6 * max(1e-30, torch.from_numpy(d[p + 'd64']).abs().max().item()) + 1e-12


def test_special_cases_are_what_they_claim():
    d = R.load()
    by = {meta['special']: (p, meta, x, sd) for p, meta, x, sd in UNITS if meta['special']}
    # (the exact answer is act(beta); the reference's float32 evaluates x * (rstd * gamma) + (beta - mean * rstd * gamma) with
    # rstd = 1 / sqrt(eps) = 316 and misses it by |x| * 316 * 2^-24: that miss is the yardstick of the GPU tests)
    p, meta, x, sd = by['one']            # H = W = 1, one channel per group: variance 0 -> leaky(beta)
    assert (R.y64(d, p) - R.act(sd['gn.bias'].double().view(1, -1, 1, 1).expand(2, -1, 1, 1), 'leaky')).abs().max().item() <= 1e-9
    p, meta, x, sd = by['const']          # group 0 (channels 0, 1) is constant -> relu(beta) there
    assert (R.y64(d, p)[:, :2] - R.act(sd['gn.bias'][:2].double().view(1, 2, 1, 1).expand(2, 2, 13, 11), 'relu')).abs().max().item() <= 1e-9
    p, meta, x, sd = by['mean']           # group 1 (channels 2, 3): mean ~1e3, spread ~1e-2
    raw = torch.nn.functional.conv2d(x.double(), sd['conv.weight'].double(), sd['conv.bias'].double())[:, 2:4]
    assert 990 < raw.mean().item() < 1010 and 1e-3 < raw.std().item() < 1e-1
    p, meta, x, sd = by['mish']
    for v in (-100., -20., -1e-3, 0., 1e-3, 19.99, 20., 20.01, 100.):
        assert bool((x == torch.tensor(v)).any()), v


# ---- (b) the surface ----------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_param_groups_are_the_reference_s():
    surf = R.surface()
    for p, meta, x, sd in UNITS:
        m = R.make_unit(meta, sd, lr=2.0, bias_lr=3.0)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in surf[p]['keys']], p
        names = {id(v): k for k, v in m.named_parameters()}
        pg = []
        m.add_param_group(pg, 0.01, 5e-4)
        got = [(names[id(g['params'][0])], g['lr'], g['base_lr'], g['weight_decay']) for g in pg]
        assert got == [tuple(t) for t in surf[p]['groups']], p
        assert all(wd == 0.0 for k, _, _, wd in got if k.split('.')[0] in ('bn', 'gn', 'af')), p      # no decay on norm scales / offsets
        m.freeze()
        assert not any(q.requires_grad for q in m.parameters())
        pg = []
        m.add_param_group(pg, 0.01, 5e-4)
        assert pg == []


def test_construction():
    from model.custom_layers import AffineChannel, Conv2dUnit, SPP
    u = Conv2dUnit(32, 64, 1, gn=1, groups=32, act='mish')
    assert isinstance(u.gn, torch.nn.GroupNorm) and (u.gn.num_groups, u.gn.num_channels) == (32, 64) and u.bn is None and u.af is None
    u = Conv2dUnit(32, 64, 1, af=1)
    assert isinstance(u.af, AffineChannel) and tuple(u.af.weight.shape) == tuple(u.af.bias.shape) == (64,)
    with pytest.raises(ValueError, match=r'num_channels \(48\) must be divisible by num_groups \(32\)'):          # what torch.nn.GroupNorm raises
        Conv2dUnit(32, 48, 1, gn=1, groups=32)
    with pytest.raises(NotImplementedError):
        Conv2dUnit(32, 64, 1, act='swish')
    assert SPP('desc').seq == 'desc'


def test_affine_channel_folds_into_the_epilogue():
    """folded() = (af.weight, af.bias + conv_bias * af.weight); the one-layer plan, replayed on the CPU, is the reference's output
    to float32 rounding (the fold multiplies the bias first: another order than conv -> + bias -> * weight)."""
    d = R.load()
    for p, meta, x, sd in UNITS:
        if meta['norm'] != 'af':
            continue
        m = R.make_unit(meta, sd)
        scale, shift = m.folded('cpu')
        assert torch.equal(scale, sd['af.weight'])
        bias = sd.get('conv.bias')
        assert torch.equal(shift, sd['af.bias'] + (bias * sd['af.weight'] if bias is not None else torch.zeros(meta['cout'])))
        b = Builder(x.shape[0], x.shape[2], x.shape[3], 'cpu')
        xin = b.new_act(x.shape[0], x.shape[2], x.shape[3], x.shape[1])
        y = m.emit(b, xin)
        assert [op['op'] for op in b.plan.ops] == (['conv', 'mish'] if meta['act'] == 'mish' else ['conv'])
        run = NormActPlanRunner(b.plan)
        run.put(xin, x.permute(0, 2, 3, 1))
        run.run(None)
        ref = R.y32(d, p)
        assert (run.get(y).permute(0, 3, 1, 2) - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item()), p


# ---- (c) plans ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfgc', [PPYOLO_2x_Config, PPYOLO_r18vd_Config])
def test_affine_channel_plan_is_the_batch_norm_plan(cfgc):
    dumps = []
    for norm in ('bn', 'affine_channel'):
        model, _ = build_model(_cfg(cfgc, norm, norm))
        dumps.append(P.dump(*P.derive(model, 8, 320)))
    assert dumps[0] == dumps[1]
    assert not any('"op": "gn"' in ln or '"op": "mish"' in ln for ln in dumps[1]['ops'])


@pytest.mark.parametrize('cfgc,bb,hd', [(PPYOLO_r18vd_Config, 'gn', 'gn'), (PPYOLO_2x_Config, 'affine_channel', 'gn'),
                                         (PPYOLO_2x_Config, 'gn', 'bn')])
def test_group_norm_plan_keeps_its_convolutions_out_of_every_link(cfgc, bb, hd):
    from ppyolo_hip import plan_links as L
    model, _ = build_model(_cfg(cfgc, bb, hd))
    plan, links, fused = P.derive(model, 8, 320)
    ops = plan.ops
    gn_ops = [op for op in ops if op['op'] == 'gn']
    assert gn_ops
    idx = L.BufferIndex(ops)
    linked = {pr for pr, _ in links} | {c for _, cons in links for c in cons} | {i for pair in fused for i in pair}

    def reads_gn(a):          # does this activation overlap the slice some 'gn' op wrote?
        return any(g['y'].buf == a.buf and g['y'].coff < a.coff + a.C and a.coff < g['y'].coff + g['y'].C for g in gn_ops)
    for g in gn_ops:
        feeders = [(i, o) for i, o in idx.writers[g['x'].buf]]
        assert len(feeders) == 1 and feeders[0][1]['op'] in ('conv', 'dcn', 'stem')
        i, f = feeders[0]
        assert f.get('act') is None and f.get('res') is None and not f.get('ups')          # the raw convolution
        assert i not in linked and f.get('pool') is None and f.get('mpool') is None and not f.get('gp_in'), (i, f['op'])
        assert [o['op'] for _, o in idx.readers[g['x'].buf]] == ['gn']                      # the scratch tensor has one reader
    for op in ops:
        ins, _ = L.op_io(op)
        if op['op'] in ('conv', 'dcn') and reads_gn(op['x']):
            assert op['amax_in_id'] is None and not L.has_f16(op)                           # readers of a 'gn' output: non-f16x2 tiles
        if op['op'] in ('avgpool', 'maxpool') and reads_gn(op['x']):
            assert op.get('owner') is None
    if (bb, hd) == ('gn', 'gn'):
        assert not links and not fused
    if bb == 'gn':          # the shortcut fold needs affine norms: conv3 keeps its residual, no wide [conv2 | shortcut] buffer
        assert sum(1 for op in gn_ops if op['res'] is not None) == (16 if cfgc is PPYOLO_2x_Config else 8)


def test_mish_keeps_the_convolution_in_front_of_it_a_launch_of_its_own():
    from model.custom_layers import Conv2dUnit
    from ppyolo_hip import ops as K
    from ppyolo_hip import plan_links as L
    b = Builder(2, 16, 16, 'cpu', skeleton=True)
    x = b.new_act(2, 16, 16, 64)
    u1, u2, u3 = (Conv2dUnit(64, 64, k, bn=1, act=a) for k, a in ((1, 'relu'), (3, 'mish'), (1, 'relu')))
    y = u3.emit(b, u2.emit(b, u1.emit(b, x)))
    ops = b.plan.ops
    assert [op['op'] for op in ops] == ['conv', 'conv', 'mish', 'conv'] and ops[1]['act'] is None and ops[2]['x'] == ops[1]['y']
    for op in ops:
        if op['op'] == 'conv':
            op['wf16'] = True
    L.assign_amax(ops)
    ops[0]['amax_in_id'] = 99          # (as if the input were tracked)
    assert ops[3]['amax_in_id'] == ops[1]['amax_out_id'] is not None          # |mish(x)| <= |x|: the block stays
    idx = L.BufferIndex(ops)
    pairs = L.split_pairs(idx, b.plan.buffers, {y.buf}, L.has_f16)
    assert [(pr is ops[0], [c is ops[1] for c in cons]) for pr, cons in pairs] == [(True, [True])]      # conv -> mish conv: its INPUT may link
    assert not L.b2b_pairs(idx, b.plan.buffers, {y.buf}, L.has_f16)


def test_shipped_plans_are_the_parent_commit_s():
    """Skeleton plans of the two shipped configurations at S = 608, 416, 320 (batch 8) with their link state and tile ids, against
    the dump tests/norm_act_plans.py took at the commit before GroupNorm / AffineChannel / Mish came in."""
    import __graft_entry__ as ge
    ge.build()
    want = json.load(open(os.path.join(R.GOLDEN, 'g23_plans_parent.json')))
    got = P.shipped_dumps()
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k]['buffers'] == want[k]['buffers'], k
        assert got[k]['ops'] == want[k]['ops'], k


def test_spp_desc_is_a_change_of_channel_offsets():
    b = Builder(1, 13, 13, 'cpu')
    wide = b.new_act(1, 13, 13, 128)
    x = b.slice(wide, 96, 32)
    y = b.spp(x, desc=True)
    assert (y.coff, y.C) == (0, 128)
    run = NormActPlanRunner(b.plan)
    xv = torch.randn(1, 32, 13, 13, generator=torch.Generator().manual_seed(5))
    run.put(x, xv.permute(0, 2, 3, 1))
    run.run(None)
    mp = torch.nn.functional.max_pool2d
    ref = torch.cat([mp(xv, 13, 1, 6), mp(xv, 9, 1, 4), mp(xv, 5, 1, 2), xv], dim=1)          # reference model/custom_layers.py:286-287
    assert torch.equal(run.get(y).permute(0, 3, 1, 2), ref)


# ---- the plans against the golden, replayed on the CPU ------------------------------------------------------------------------
@pytest.mark.parametrize('tag,cfgc,bb,hd', [('r18vd_64', PPYOLO_r18vd_Config, 'gn', 'gn'), ('r50vd_96', PPYOLO_2x_Config, 'affine_channel', 'gn')])
def test_model_plans_replayed_on_the_cpu(tag, cfgc, bb, hd):
    """Bound: these plans run the reference's own ATen ops in another grouping (folded affine, fused shortcut), so they differ from
    the golden by float32 rounding amplified through the GroupNorm layers; 1e-3 of the tensor's maximum separates that from any
    mistake of the emission (a wrong slice, a residual on the wrong side of the norm), which is of order 1."""
    d = R.load('g23_norm_act_' + tag)
    S, N, seed, iseed = [int(v) for v in d['meta']]
    model, _ = build_model(_cfg(cfgc, bb, hd), seed)
    plan = build_plan(model, N, S, S, 'cpu')
    feats, outs, _ = NormActPlanRunner(plan).run(synth.synth_images(N, S, seed=iseed))
    for kind, got in (('feat', feats), ('out', outs)):
        for i, t in enumerate(got):
            ref = torch.from_numpy(d['%s%d' % (kind, i)])
            assert t.shape == ref.shape
            assert (t - ref).abs().max().item() <= 1e-3 * max(1.0, ref.abs().max().item()), (tag, kind, i)


# ---- (d) training stays BatchNorm only ----------------------------------------------------------------------------------------
def test_train_step_refuses_other_norms_by_name():
    from ppyolo_hip.train import check_bn_only
    model, _ = build_model(PPYOLO_r18vd_Config())
    check_bn_only(model)
    model, _ = build_model(_cfg(PPYOLO_r18vd_Config, 'bn', 'gn'))
    with pytest.raises(PPYoloHipError, match=r'head\.detection_blocks\.0\.layers\.\d+ \(yolo_block\.0\.\S+\) holds GroupNorm'):
        check_bn_only(model)
    model, _ = build_model(_cfg(PPYOLO_r18vd_Config, 'affine_channel', 'bn'))
    with pytest.raises(PPYoloHipError, match=r'backbone\.stage1_conv1_1 \(conv1_1\) holds AffineChannel'):
        check_bn_only(model)
    model, _ = build_model(PPYOLO_r18vd_Config())
    model.head.yolo_output_convs[0].act_name = 'mish'
    with pytest.raises(PPYoloHipError, match='Mish'):
        check_bn_only(model)
