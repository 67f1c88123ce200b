"""GroupNorm / AffineChannel / Mish on the MI355X: ppy_group_norm_f32 and ppy_mish_f32 called directly, the unit and block cases of
tests/golden/g23_norm_act*.npz through Conv2dUnit.forward and through plans with channel-sliced destinations, and the two model
cases in graph and eager mode.

Bounds.  AffineChannel and bn + mish cases: `close(rel=2e-5)` of tests/test_gpu_ops.py.  GroupNorm divides by the group's spread,
so that bound does not transfer; a gn case is judged against the golden's float64 output: max |got - y64| <= K_GN * max |y32 - y64|,
where y32 is the REFERENCE's own float32 output -- the yardstick is the reference, not the code under test.  Every ratio is
printed before it is asserted (profiles/norm_act_parity.txt holds the worst per family as measured on the MI355X).
"""
import numpy as np
import pytest
import torch

import norm_act_ref as R
from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from ppyolo_hip import synth

pytestmark = pytest.mark.gpu

# Worst ratio measured on the MI355X over every gn case, rounded up to the next integer, plus one (profiles/norm_act_parity.txt).
K_GN = 3
ULP = 2.0 ** -24
UNITS = R.unit_cases()
_IDS = [c[0] + (c[1]['special'] or '%s_%s' % (c[1]['norm'], c[1]['act'])) for c in UNITS]


def close(a, b, rel=2e-5, what=''):          # tests/test_gpu_ops.py
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= rel * scale, '%s: max abs err %.3e (scale %.3e)' % (what, err, scale)
    return err / scale


def judge_gn(family, what, got, d, p, key='y32', dkey='d64'):
    e_got, e_ref = R.err_ratio(got, d, p, key, dkey)
    print('norm_act_parity %-6s %-28s err %.3e  reference %.3e  ratio %.3f' % (family, what, e_got, e_ref, e_got / max(e_ref, 1e-300)))
    assert e_got <= K_GN * e_ref, '%s: %.3e against float64, the reference\'s float32 %.3e (ratio %.2f > %d)' % (what, e_got, e_ref, e_got / max(e_ref, 1e-300), K_GN)


def judge(family, what, got, d, p, gn):
    if gn:
        judge_gn(family, what, got, d, p)
    else:
        close(got, R.y32(d, p), what=what)


# ---- the kernels, called directly -----------------------------------------------------------------------------------------------
def _views(N, H, W, C, gen, up=1):
    """x in a wider buffer at a channel offset, y in another one (other pitch, other offset), a residual in a third."""
    from ppyolo_hip import ops as K
    xb = torch.randn(N, H, W, C + 36, generator=gen)
    xb[1:] = xb[1:] * 2.5 - 0.75
    rb = torch.randn(N, H, W, C + 8, generator=gen)
    yb = torch.full((N, up * H, up * W, C + 20), 7.25)
    xv, rv, yv = K.View(xb.cuda(), 32, C), K.View(rb.cuda(), 4, C), K.View(yb.cuda(), 16, C)
    return xb[..., 32:32 + C], rb[..., 4:4 + C], xv, rv, yv


def _gn_ref(x, gamma, beta, groups, res, act, eps=1e-5):
    """float64, NHWC in and out."""
    y = R.group_norm_two_pass(x.double().permute(0, 3, 1, 2).contiguous(), gamma.double(), beta.double(), groups, eps)
    pre = y + (res.double().permute(0, 3, 1, 2) if res is not None else 0.0)
    return R.act(pre, act).permute(0, 2, 3, 1), y.abs().max().item() + (res.abs().max().item() if res is not None else 0.0)


GN_SHAPES = [  # N, H, W, C, groups, act, residual
    (2, 13, 11, 64, 32, 'relu', True),          # C / groups = 2: a 16-byte access spans two groups; five pixel chunks
    (2, 5, 7, 256, 32, 'leaky', False),         # C / groups = 8, one chunk
    (1, 40, 40, 96, 32, 'mish', True),          # C / groups = 3 (the general path), 24 channel quads on 32 lanes
    (2, 70, 70, 32, 4, None, False),            # 126 chunks of 39 pixels, the last one short; C / groups = 8 over 8 quads
    (3, 3, 3, 2048, 32, 'relu', True),          # eight passes of the 64 channel-quad lanes
    (2, 1, 1, 32, 32, 'leaky', False),          # one element per group: variance 0, the output is act(beta)
]


@pytest.mark.parametrize('N,H,W,C,groups,act,with_res', GN_SHAPES)
def test_group_norm_kernel(N, H, W, C, groups, act, with_res):
    """Bound: the apply pass is d = fl(x - mean) (mean a double), d * rstd * gamma + beta [+ res] in float32 -- five roundings of
    intermediates no larger than S = max|xhat gamma + beta| + max|res|, rstd itself off by one -- and Mish adds expf (1 ulp = 2^-23)
    and five more roundings with |mish'| <= 1.09: 16 * 2^-24 * S covers both, and the statistics (double sums) add nothing visible."""
    from ppyolo_hip import ops as K
    gen = torch.Generator().manual_seed(1000 + C + H)
    x, res, xv, rv, yv = _views(N, H, W, C, gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    ref, S = _gn_ref(x, gamma, beta, groups, res if with_res else None, act)
    K.group_norm(xv, gamma.cuda(), beta.cuda(), groups, 1e-5, yv, act, rv if with_res else None)
    torch.cuda.synchronize()
    got = yv.dense().cpu()
    err = (got.double() - ref).abs().max().item()
    print('group_norm %s: err %.3e, bound %.3e' % ((N, H, W, C, groups, act), err, 16 * ULP * max(1.0, S)))
    assert err <= 16 * ULP * max(1.0, S)
    full = yv.t.cpu()
    assert bool((full[..., :16] == 7.25).all()) and bool((full[..., 16 + C:] == 7.25).all())          # nothing outside the slice
    first = got.clone()
    yv.t.fill_(7.25)
    K.group_norm(xv, gamma.cuda(), beta.cuda(), groups, 1e-5, yv, act, rv if with_res else None)
    torch.cuda.synchronize()
    assert torch.equal(yv.dense().cpu(), first)          # bit-identical from run to run: no atomics, a fixed order
    # the 2 x 2 nearest-upsampled destination: the plain result, repeated
    _, _, _, _, yu = _views(N, H, W, C, gen, up=2)
    K.group_norm(xv, gamma.cuda(), beta.cuda(), groups, 1e-5, yu, act, rv if with_res else None, upsample2x=True)
    torch.cuda.synchronize()
    assert torch.equal(yu.dense().cpu(), first.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
    fu = yu.t.cpu()
    assert bool((fu[..., :16] == 7.25).all()) and bool((fu[..., 16 + C:] == 7.25).all())


def test_group_norm_kernel_large_mean():
    """A group with mean 1e3 and spread 1e-2: E[x^2] - E[x]^2 in float32 would leave no digit of the variance.  Against float64 on
    the SAME float32 input the only errors are those of the apply pass (bound as above)."""
    from ppyolo_hip import ops as K
    gen = torch.Generator().manual_seed(77)
    N, H, W, C, groups = 2, 13, 11, 64, 32
    x, _, xv, _, yv = _views(N, H, W, C, gen)
    xb = xv.t.cpu()
    xb[..., 32 + 2:32 + 4] = 1000.0 + 1e-2 * xb[..., 32 + 2:32 + 4]
    xv.t.copy_(xb)
    x = xb[..., 32:32 + C]
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    ref, S = _gn_ref(x, gamma, beta, groups, None, None)
    K.group_norm(xv, gamma.cuda(), beta.cuda(), groups, 1e-5, yv, None)
    torch.cuda.synchronize()
    err = (yv.dense().cpu().double() - ref).abs().max().item()
    print('group_norm large mean: err %.3e, bound %.3e' % (err, 16 * ULP * max(1.0, S)))
    assert err <= 16 * ULP * max(1.0, S)


def test_group_norm_kernel_rejects_bad_arguments():
    from ppyolo_hip import ops as K
    from ppyolo_hip._lib import PPYoloHipError
    gen = torch.Generator().manual_seed(3)
    _, _, xv, rv, yv = _views(1, 4, 4, 64, gen)
    g = torch.ones(64).cuda()
    with pytest.raises(PPYoloHipError):
        K.group_norm(xv, g, g, 24, 1e-5, yv)                                          # 64 % 24
    with pytest.raises(PPYoloHipError, match='workspace'):
        K.group_norm(xv, g, g, 32, 1e-5, yv, ws=torch.empty(16, device='cuda'))


@pytest.mark.parametrize('N,H,W,C', [(2, 13, 11, 64), (1, 3, 4, 32), (2, 9, 9, 260)])
def test_mish_kernel(N, H, W, C):
    """Elementwise bound: expf is good to 1 ulp (2^-23), n = e (e + 2) carries it twice plus two roundings, n / (n + 2) and the
    product with x three more: <= 11 * 2^-24 relative, asserted as 16; results below 1e-37 may be flushed to zero."""
    from ppyolo_hip import ops as K
    gen = torch.Generator().manual_seed(C)
    buf = torch.randn(N, H, W, C + 12, generator=gen) * 8.0
    probe = torch.tensor([-100., -20., -1e-3, 0., 1e-3, 19.99, 20., 20.01, 100., -87., 88., 9.02])
    buf[0, :, :, 8:20] = probe
    v = K.View(buf.cuda(), 8, C)
    ref = R.mish(buf[..., 8:8 + C].double())
    K.mish(v)
    torch.cuda.synchronize()
    out = v.t.cpu()
    got = out[..., 8:8 + C].double()
    assert bool(((got - ref).abs() <= 16 * ULP * ref.abs() + 1e-37).all()), ((got - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
    assert torch.equal(out[..., :8], buf[..., :8]) and torch.equal(out[..., 8 + C:], buf[..., 8 + C:])          # in place, on the slice only
    assert torch.equal(got[0, 0, 0, 5:9].float(), torch.tensor([19.99, 20., 20.01, 100.]) * torch.tanh(torch.nn.functional.softplus(
        torch.tensor([19.99, 20., 20.01, 100.])))), 'x > 20 gives x; just below it tanh(softplus(x)) rounds to 1'


# ---- unit cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', UNITS, ids=_IDS)
def test_unit_forward_and_sliced_plan(case):
    """Conv2dUnit.forward (engine.run_single), then the same unit in a one-layer plan whose destination is a channel slice of a
    wider buffer (ld > C): the same values, and nothing outside the slice."""
    from ppyolo_hip.engine import Builder, HipExecutor
    p, meta, x, sd = case
    d = R.load()
    gn = meta['norm'] == 'gn'
    fam = meta['special'] or meta['norm']
    m = R.make_unit(meta, sd).cuda()
    y = m(x.cuda())
    judge(fam, p + 'forward', y, d, p, gn)
    N, Cin, H, W = x.shape
    b = Builder(N, H, W, torch.device('cuda'))
    xin = b.new_act(N, H, W, Cin)
    Ho, Wo = y.shape[2], y.shape[3]
    wide = b.new_act(N, Ho, Wo, meta['cout'] + 48)
    out = m.emit(b, xin, out=b.slice(wide, 16, meta['cout']))
    ex = HipExecutor(b.plan, 'cuda', use_graph=False)
    ex.bufs[xin.buf].copy_(x.permute(0, 2, 3, 1))
    ex.bufs[wide.buf].fill_(-3.5)
    ex.run()
    torch.cuda.synchronize()
    assert torch.equal(ex.view(out).dense().permute(0, 3, 1, 2), y)
    full = ex.bufs[wide.buf].cpu()
    assert bool((full[..., :16] == -3.5).all()) and bool((full[..., 16 + meta['cout']:] == -3.5).all())


# ---- block cases ----------------------------------------------------------------------------------------------------------------
def _run_plan(b, feeds):
    from ppyolo_hip.engine import HipExecutor
    ex = HipExecutor(b.plan, 'cuda', use_graph=False)
    for a, t in feeds:
        ex.bufs[a.buf][..., a.coff:a.coff + a.C] = t.permute(0, 2, 3, 1).cuda()
    ex.run()
    torch.cuda.synchronize()
    return ex


@pytest.mark.parametrize('which', ['b0_identity', 'b1_convblock'])
def test_bottleneck_blocks_with_group_norm(which):
    """relu(gn(conv3) + shortcut): the residual is added after the norm."""
    from model.resnet_vd import ConvBlock, IdentityBlock
    from ppyolo_hip.engine import Builder
    d = R.load('g23_norm_act_blocks')
    p = which[:3]
    blk = (IdentityBlock(128, [32, 32, 128], 0, 1, 0, False, 0., 1.) if p == 'b0_' else ConvBlock(64, [32, 32, 128], 0, 1, 0, False, 0., 1., stride=2))
    blk.load_state_dict(R.state(d, p), strict=True)
    blk = blk.eval().cuda()
    x = torch.from_numpy(d[p + 'x'])
    b = Builder(x.shape[0], x.shape[2], x.shape[3], torch.device('cuda'))
    xin = b.new_act(x.shape[0], x.shape[2], x.shape[3], x.shape[1])
    y = blk.emit(b, xin)
    assert [op['op'] for op in b.plan.ops].count('gn') == (3 if p == 'b0_' else 4)
    ex = _run_plan(b, [(xin, x)])
    judge_gn('block', which, ex.view(y).dense().permute(0, 3, 1, 2), d, p)


def test_head_route_with_group_norm():
    """gn conv -> nearest x2 -> concat: the 'gn' op stores to the upsampled slice in front of the backbone's map."""
    from ppyolo_hip.engine import Builder
    d = R.load('g23_norm_act_blocks')
    x, skip = torch.from_numpy(d['b2_x']), torch.from_numpy(d['b2_skip'])
    meta = dict(norm='gn', act='leaky', cin=64, cout=32, k=1, stride=1, bias=False, groups=32)
    m = R.make_unit(meta, R.state(d, 'b2_')).cuda()
    N, _, H, W = x.shape
    b = Builder(N, H, W, torch.device('cuda'))
    xin = b.new_act(N, H, W, 64)
    wide = b.new_act(N, 2 * H, 2 * W, 64)
    m.emit(b, xin, out=b.slice(wide, 0, 32), ups=True)
    ex = _run_plan(b, [(xin, x), (b.slice(wide, 32, 32), skip)])
    judge_gn('block', 'b2_route', ex.view(wide).dense().permute(0, 3, 1, 2), d, 'b2_')


def test_dcn_unit_with_group_norm():
    d = R.load('g23_norm_act_blocks')
    from model.custom_layers import Conv2dUnit
    m = Conv2dUnit(32, 32, 3, stride=1, gn=1, groups=4, act='relu', use_dcn=True)
    m.load_state_dict(R.state(d, 'b3_'), strict=True)
    y = m.eval().cuda()(torch.from_numpy(d['b3_x']).cuda())
    judge_gn('block', 'b3_dcn', y, d, 'b3_')


# ---- model cases ----------------------------------------------------------------------------------------------------------------
def _cfg(cfgc, backbone, head):
    cfg = cfgc()
    cfg.backbone['norm_type'], cfg.head['norm_type'] = backbone, head
    return cfg


MODELS = [('r18vd_64', PPYOLO_r18vd_Config, 'gn', 'gn'), ('r50vd_96', PPYOLO_2x_Config, 'affine_channel', 'gn')]


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('tag,cfgc,bb,hd', MODELS)
def test_model_feature_maps_and_head_outputs(tag, cfgc, bb, hd, graph):
    from ppyolo_hip.engine import HipExecutor
    from ppyolo_hip.runtime import build_plan
    d = R.load('g23_norm_act_' + tag)
    S, N, seed, iseed = [int(v) for v in d['meta']]
    model, _ = build_model(_cfg(cfgc, bb, hd), seed, 'cuda')
    plan = build_plan(model, N, S, S, torch.device('cuda'))
    ex = HipExecutor(plan, 'cuda', use_graph=graph)
    ex.set_inputs(synth.synth_images(N, S, seed=iseed).cuda(), synth.synth_im_size(N).cuda())
    ex.run()
    ex.run()
    torch.cuda.synchronize()
    for i, a in enumerate(plan.feats):
        got = ex.view(a).dense().permute(0, 3, 1, 2)
        if bb == 'gn':
            judge_gn('model', '%s feat%d' % (tag, i), got, d, '', 'feat%d' % i, 'feat%d_d64' % i)
        else:          # AffineChannel only: the bound of the g6 tests (tests/test_gpu_model.py)
            close(got, torch.from_numpy(d['feat%d' % i]), rel=1e-4, what='%s feat%d' % (tag, i))
    for i, a in enumerate(plan.head_outs):
        judge_gn('model', '%s out%d' % (tag, i), ex.view(a).dense().permute(0, 3, 1, 2), d, '', 'out%d' % i, 'out%d_d64' % i)


@pytest.mark.parametrize('graph', ['0', '1'], ids=['eager', 'graph'])
@pytest.mark.parametrize('tag,cfgc,bb,hd', MODELS)
def test_model_detections(tag, cfgc, bb, hd, graph, monkeypatch, capsys):
    """model(x, im_size), forward_padded and in_flight against the golden's rows: the same detections in the same order (labels
    equal), scores <= 1e-4 (the literal bar of g7), and -- GroupNorm is involved in both models -- every box no further from the
    reference's float64 rows than K_GN times the reference's own float32 rows are.  The literal 1e-3 px of g7 against the float32
    rows is REPORTED, not asserted, with the reference-against-itself count beside it (as bench.py's parity_note does): measured
    on the MI355X, r18vd_64 (gn / gn, boxes of up to 640 px): 4 of 200 boxes beyond 1e-3 px, the worst 1.22e-3 px, where the
    reference's float32 rows are within 7.6e-4 px of its float64 rows (0 of 200 beyond) -- two float32-grade evaluations of the
    same boxes differ by the sum of their distances to the exact one.  r50vd_96 (affine_channel / gn) yields no detection on the
    synthetic weights: both sides return the empty-result row."""
    monkeypatch.setenv('PPYOLO_HIP_GRAPH', graph)
    d = R.load('g23_norm_act_' + tag)
    S, N, seed, iseed = [int(v) for v in d['meta']]
    model, _ = build_model(_cfg(cfgc, bb, hd), seed, 'cuda')
    x, ims = synth.synth_images(N, S, seed=iseed).cuda(), torch.from_numpy(d['im_size']).cuda()
    preds = model(x, ims)
    dets, cnt, keep = model.forward_padded(x, ims)
    lines = []
    for i in range(N):
        ref, ref64 = torch.from_numpy(d['pred%d' % i]), torch.from_numpy(d['pred%d_y64' % i])
        p = preds[i].cpu()
        rows = 0 if ref[0, 0] == -1 else ref.shape[0]          # (no detection: one row of -1, reference model/head.py)
        assert p.shape == ref.shape and int(cnt[i]) == rows
        assert rows == 0 or torch.equal(dets[i, :rows].cpu(), p)
        assert torch.equal(p[:, 0], ref[:, 0]), 'image %d: labels / order differ' % i
        assert ref64.shape == ref.shape and torch.equal(ref64[:, 0].float(), ref[:, 0]), 'fixture: the float64 rows are other detections'
        es, eb = (p[:, 1] - ref[:, 1]).abs().max().item(), (p[:, 2:] - ref[:, 2:]).abs().max(dim=1).values
        own = (ref[:, 2:].double() - ref64[:, 2:]).abs().max(dim=1).values
        mine64 = (p[:, 2:].double() - ref64[:, 2:]).abs().max().item()
        lines.append('norm_act_parity detect %s image %d: %d rows, score err %.2e, box err %.2e px, %d beyond 1e-3 px (the reference\'s float32 '
                     'against its float64: %d beyond, max %.2e px); against float64: %.2e px' % (
                         tag, i, rows, es, eb.max().item(), int((eb > 1e-3).sum()), int((own > 1e-3).sum()), own.max().item(), mine64))
        assert es <= 1e-4, 'image %d scores' % i
        assert mine64 <= K_GN * own.max().item(), lines[-1]
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    lanes = model.in_flight(depth=2)
    t = lanes.submit(x, ims)
    d2, c2, _ = t.padded()
    assert torch.equal(c2.cpu(), cnt.cpu()) and torch.equal(d2.cpu(), dets.cpu())
    for a, b in zip(t.result(), preds):
        assert torch.equal(a, b)
