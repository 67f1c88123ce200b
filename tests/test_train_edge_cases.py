"""The edge table of tests/train_edge_cases.py is what it says, fair and sharp -- no GPU: with plain torch float32 on the CPU standing
in for the kernels, (1) every case keeps its promise (restated launch arithmetic, value edges, ties), (2) every case passes the
launch-level float64 checkers of tests/launch_replay.py at their own bounds, ratio <= 1 (a condition, not a measurement: a case
a correct float32 implementation fails would be replaced, never given a wider bound), (3) one planted fault per family fails the
named check on an edge case, and (4) every checker of the replay has a case or sits on the table's exempt list."""
import pytest
import torch
import torch.nn.functional as F

import launch_replay as lr
import train_edge_cases as tec
from ppyolo_hip import ops
from train_edge_cases import CASES, dense

AMAX = ops.AMAX_FLOATS_PER_IMAGE


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


_act = tec.act_f32


def _slope(y, act, fault=None):
    if act is None:
        return torch.ones_like(y)
    pos = (y >= 0) if fault == 'slope 1 at zero' else (y > 0)
    return torch.where(pos, torch.ones_like(y), torch.full_like(y, 0.0 if act == 'relu' else 0.1))


def _track(block, out, fault=None, hw=None, ppb=None):
    """max|out| per image into slot 0 of the block.  Fault: in every workgroup (ppb pixels) that straddles two images, the maximum
    over the second image's pixels is credited to the first image."""
    N = out.shape[0]
    a = out.abs().reshape(N, -1, out.shape[-1])
    m = a.reshape(N, -1).amax(dim=1)
    if fault == 'maximum credited to the wrong image':
        m = m.clone()
        for n in range(1, N):
            head = (n * hw // ppb + 1) * ppb - n * hw            # pixels of image n in the workgroup it shares with image n - 1
            if 0 < head < ppb:
                m[n - 1] = torch.maximum(m[n - 1], a[n, :head].max())
                m[n] = a[n, head:].max()
    b = block.view(N, AMAX)
    b[:, 0] = torch.maximum(b[:, 0], m)


def _route(x, dy, k, stride, pad, last):
    """Max-pool backward by explicit routing to the first (or, the fault, the last) maximum of every window."""
    N, H, W, C = x.shape
    first, lastp = tec.first_last_argmax(x, k, stride, pad)
    j = lastp if last else first                                          # [N, C, L] position inside the window
    Ho, Wo = dy.shape[1], dy.shape[2]
    ho = torch.arange(Ho).repeat_interleave(Wo).view(1, 1, -1)
    wo = torch.arange(Wo).repeat(Ho).view(1, 1, -1)
    idx = (ho * stride - pad + j // k) * W + (wo * stride - pad + j % k)
    dx = torch.zeros(N, C, H * W)
    dx.scatter_add_(2, idx, _nchw(dy).reshape(N, C, -1))
    return _nhwc(dx.view(N, C, H, W))


# ---- float32 stand-ins: kw -> what the op returns, results written where the op writes them ---------------------------------------
def s_bn_train_stats(kw, fault=None):
    x = dense(kw['x']).reshape(-1, kw['x'].C)
    if fault == 'last slice dropped':
        _, pps, sl = tec.bn_slices(x.shape[0], x.shape[1])
        x = x[:(sl - 1) * pps]
    P = x.shape[0]
    m = x.mean(0)
    var = (x * x).mean(0) - m * m if fault == 'one-pass variance' else ((x - m) ** 2).mean(0)
    kw['mean'].copy_(m)
    kw['invstd'].copy_(1.0 / torch.sqrt(var + kw['eps']))
    mom = kw['momentum']
    if kw['running_mean'] is not None:
        kw['running_mean'].copy_((1 - mom) * kw['running_mean'] + mom * m)
    if kw['running_var'] is not None:
        kw['running_var'].copy_((1 - mom) * kw['running_var'] + mom * (var * P / (P - 1) if P > 1 else var))


def s_bn_train_stats_merge(kw, fault=None):
    C, sl = kw['mean'].numel(), kw['slices']
    p = kw['partials'][:sl * C * 3].view(sl, C, 3)
    n, m, m2 = p[..., 0], p[..., 1], p[..., 2]
    nt = n.sum(0)
    mean = (n * m).sum(0) / nt
    M2 = (m2 + n * (m - mean) ** 2).sum(0)
    kw['mean'].copy_(mean)
    kw['invstd'].copy_(1.0 / torch.sqrt(M2 / nt + kw['eps']))
    mom = kw['momentum']
    kw['running_mean'].copy_((1 - mom) * kw['running_mean'] + mom * mean)
    kw['running_var'].copy_((1 - mom) * kw['running_var'] + mom * M2 / (nt - 1).clamp_min(1))


def s_bn_train_apply(kw, fault=None):
    x, y = kw['x'], kw['y']
    z = (dense(x) - kw['mean']) * (kw['invstd'] * kw['gamma']) + kw['beta']
    if kw['residual'] is not None:
        z = z + dense(kw['residual'])
    out = _act(z, kw['act'])
    dense(y).copy_(out)
    if fault == 'channel past the slice':
        y.t[..., y.coff + y.C] = 0.0
    if kw['amax_out'] is not None:
        hw = x.H * x.W
        _track(kw['amax_out'], out, fault, hw, tec.apply_ppb(x.N * hw, x.C, hw))


def s_bn_train_bwd(kw, fault=None):
    x = kw['x']
    C = x.C
    P = x.N * x.H * x.W
    dz = (dense(kw['dy']) * _slope(dense(kw['y']), kw['act'], fault)).reshape(P, C)
    xh = (dense(x).reshape(P, C) - kw['mean']) * kw['invstd']
    sa, sb = dz.sum(0), (dz * xh).sum(0)
    kw['dbeta'].copy_(sa)
    kw['dgamma'].copy_(sb)
    dx = (kw['gamma'] * kw['invstd'] * (dz - (sa + xh * sb) * (1.0 / P))).view(x.N, x.H, x.W, C)
    dense(kw['dx']).copy_(dx)
    if kw['amax_dx'] is not None:
        hw = x.H * x.W
        _track(kw['amax_dx'], dx, fault, hw, tec.apply_ppb(P, C, hw))


def s_act_bwd(kw, fault=None):
    dense(kw['dx']).copy_(dense(kw['dy']) * _slope(dense(kw['y']), kw['act'], fault))


def s_add_inplace(kw, fault=None):
    dense(kw['dst']).add_(dense(kw['src']))


def s_dropblock_apply(kw, fault=None):
    dense(kw['y']).copy_(dense(kw['x']) * kw['mask'] * kw['scale'])


def s_upsample2x(kw, fault=None):
    dense(kw['y']).copy_(dense(kw['x']).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))


def s_upsample2x_bwd(kw, fault=None):
    dy, dx = dense(kw['dy']), kw['dx']
    q = dy.reshape(dx.N, dx.H, 2, dx.W, 2, dx.C)
    r = (q[:, :, 0, :, 0] + q[:, :, 0, :, 1]) + (q[:, :, 1, :, 0] + q[:, :, 1, :, 1])
    if kw['accumulate'] and fault != 'accumulate ignored':
        r = r + dense(dx)
    dense(dx).copy_(r)


def s_avgpool2x2(kw, fault=None):
    dense(kw['y']).copy_(_nhwc(F.avg_pool2d(_nchw(dense(kw['x'])), 2, 2)))


def s_avgpool2x2_bwd(kw, fault=None):
    dy, dx = dense(kw['dy']), kw['dx']
    up = 0.25 * dy.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    if fault == 'odd last row filled':
        up = F.pad(_nchw(up), (0, dx.W - up.shape[2], 0, dx.H - up.shape[1]), mode='replicate')
        up = _nhwc(up)
    out = torch.zeros(dx.N, dx.H, dx.W, dx.C)
    out[:, :up.shape[1], :up.shape[2]] = up
    dense(dx).copy_(out)


def s_zero_insert(kw, fault=None):
    dy, up, s = kw['dy'], kw['up'], kw['stride']
    out = torch.zeros(up.N, up.H, up.W, up.C)
    out[:, 0:dy.H * s:s, 0:dy.W * s:s] = dense(dy)
    dense(up).copy_(out)


def s_channel_sum(kw, fault=None):
    kw['out'].copy_(dense(kw['dy']).reshape(-1, kw['dy'].C).sum(0))


def s_sgd_momentum(kw, fault=None):
    p, g, v = kw['param'], kw['grad'], kw['velocity']
    d = g + kw['weight_decay'] * p
    v.copy_(d if kw['first_step'] else kw['momentum'] * v + d)
    p.sub_(kw['lr'] * v)


def ema_reference(shadow, param, step, ema_decay):
    """model/EMA.py in numpy float32: decay * shadow + (1 - decay) * param, three roundings, no fma."""
    import numpy as np
    decay = min(ema_decay, (1 + step) / (10 + step))
    a = np.float32(decay) * shadow.numpy()
    b = np.float32(1 - decay) * param.numpy()
    return decay, torch.from_numpy(a + b)


def s_ema_update(kw, fault=None):
    decay, s = ema_reference(kw['shadow'], kw['param'], kw['step'], kw['ema_decay'])
    kw['shadow'].copy_(s)
    return decay


def s_maxpool3x3s2(kw, fault=None):
    dense(kw['y']).copy_(_nhwc(F.max_pool2d(_nchw(dense(kw['x'])), 3, 2, 1)))


def s_maxpool3x3s2_bwd(kw, fault=None):
    x, dy = dense(kw['x']), dense(kw['dy'])
    if fault == 'last maximum':
        dx = _route(x, dy, 3, 2, 1, True)
    else:                                   # torch autograd = the reference's backward: the first maximum in scan order
        xr = _nchw(x).clone().requires_grad_(True)
        with torch.enable_grad():
            F.max_pool2d(xr, 3, 2, 1).backward(_nchw(dy))
        dx = _nhwc(xr.grad)
    dense(kw['dx']).copy_(dx)


def s_spp(kw, fault=None):
    x = _nchw(dense(kw['x']))
    for k, key in ((5, 'y5'), (9, 'y9'), (13, 'y13')):
        dense(kw[key]).copy_(_nhwc(F.max_pool2d(x, k, 1, k // 2)))


def s_spp_bwd(kw, fault=None):
    x, dy = dense(kw['x']), dense(kw['dy'])
    C = x.shape[-1]
    if fault == 'last maximum':
        dx = dy[..., :C].clone()
        for j, k in enumerate((5, 9, 13)):
            dx = dx + _route(x, dy[..., (j + 1) * C:(j + 2) * C], k, 1, k // 2, True)
    else:
        xr = _nchw(x).clone().requires_grad_(True)
        with torch.enable_grad():
            torch.cat([xr] + [F.max_pool2d(xr, k, 1, k // 2) for k in (5, 9, 13)], dim=1).backward(_nchw(dy))
        dx = _nhwc(xr.grad)
    dense(kw['dx']).copy_(dx)


def s_dropblock_mask(kw, fault=None):
    N, H, W, C = kw['mask'].shape
    m = _nhwc(tec.dropblock_mask_reference(N, H, W, C, kw['keep_prob'], kw['seed']))
    kw['mask'].copy_(m)
    kw['scale'].fill_(m.numel() / float(m.sum()))


def _conv32(x, w_krsc, stride, pad):
    return _nhwc(F.conv2d(_nchw(x), w_krsc.permute(0, 3, 1, 2), None, stride, pad))


def _one_slice_partials(part, y):
    """(n, mean, M2) of y [.., K] as ONE slice."""
    yy = y.reshape(-1, y.shape[-1])
    m = yy.mean(0)
    part[:yy.shape[1] * 3].view(-1, 3).copy_(torch.stack([torch.full_like(m, float(yy.shape[0])), m, ((yy - m) ** 2).sum(0)], dim=1))
    return 1


def s_conv2d_bn_act(kw, fault=None):
    z = _conv32(dense(kw['x']), kw['w_krsc'], kw['stride'], kw['pad']) * kw['scale'] + kw['shift']
    if kw['residual'] is not None:
        z = z + dense(kw['residual'])
    out = _act(z, kw['act'])
    dense(kw['y']).copy_(out)
    if kw.get('amax_out') is not None:
        _track(kw['amax_out'], out)


def s_conv2d_train_fwd(kw, fault=None):
    y = _conv32(dense(kw['x']), kw['w_krsc'], kw['stride'], kw['pad']) + kw['bias']
    dense(kw['y']).copy_(y)
    return _one_slice_partials(kw['partials'], y)


def s_conv1x1_stats(kw, fault=None):
    return _one_slice_partials(kw['partials'], _conv32(dense(kw['x']), kw['_w_krsc'], 1, 0) + kw['bias'])


def s_conv1x1_bn_apply(kw, fault=None):
    z = (_conv32(dense(kw['x']), kw['_w_krsc'], 1, 0) + kw['bias'] - kw['mean']) * (kw['invstd'] * kw['gamma']) + kw['beta']
    if kw['residual'] is not None:
        z = z + dense(kw['residual'])
    out = _act(z, kw['act'])
    dense(kw['y']).copy_(out)
    _track(kw['amax_out'], out)


def s_conv2d_dgrad(kw, fault=None):
    w = kw['prep']['w'] if 'prep' in kw else kw['w_krsc']
    dense(kw['dx']).copy_(_nhwc(F.conv_transpose2d(_nchw(dense(kw['dy'])), w.permute(0, 3, 1, 2), padding=kw['pad'])))


s_conv2d_dgrad_prepared = s_conv2d_dgrad


def s_conv2d_wgrad(kw, fault=None):
    dw = kw['dw_krsc']
    K, R, S, C = dw.shape
    dw.copy_(torch.nn.grad.conv2d_weight(_nchw(dense(kw['x'])), (K, C, R, S), _nchw(dense(kw['dy'])), stride=kw['stride'],
                                         padding=kw['pad']).permute(0, 2, 3, 1))
    if fault == 'off-centre tap non-zero':
        dw[K - 1, 0, 2, C - 1] = 1e-6 * float(dw.abs().max())
    if fault == 'off-centre tap a denormal':          # (exactly 0 is demanded: no operand-scale floor on a tap that reads padding only)
        dw[0, 2, 1, 0] = tec.DENORMAL


STANDINS = {k[2:]: v for k, v in list(globals().items()) if k.startswith('s_')}


def call_args(kw):
    """The arguments of the call: kw without the table's private '_' keys."""
    return {k: v for k, v in kw.items() if not k.startswith('_')}


def weight_cache_stub(kw):
    """What Replay needs of a TrainStep to find the fp32 master behind f16x2 planes: `_wcache`."""
    import types
    if '_w_krsc' not in kw:
        return None
    return types.SimpleNamespace(_wcache={0: {'f16': kw['w_f16'], 'krsc': kw['_w_krsc']}})


def run_case(case, fault=None):
    kw = case.build()
    rep = lr.Replay(ops, weight_cache_stub(kw))
    fn = STANDINS[case.op]
    rep.run(case.op, rep.bind(getattr(ops, case.op), **call_args(kw)), lambda: fn(kw, fault))
    return rep, kw


# ---- (1) promises, (2) fairness ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_case_keeps_its_promise_and_a_float32_implementation_passes(name):
    case = CASES[name]
    kw = case.build()
    r = case.promise(kw)                     # (every case has one: the table's constructor demands it)
    assert r is None or r, '%s does not hold: %s' % (name, case.why)
    for v in kw.values():
        t = v.t if isinstance(v, ops.View) else v
        if torch.is_tensor(t) and t.is_floating_point():
            assert bool(torch.isfinite(t).all()), name
    rep, _ = run_case(case)
    assert not rep.failures, rep.report(name)
    assert rep.census and rep.census[-1]['checks'] and rep.census[-1]['ratio'] <= 1.0, rep.report(name)


def test_ema_standin_is_three_roundings():
    """The numpy float32 expression the GPU test holds ema_update to differs from an fma / float64 evaluation somewhere."""
    kw = CASES['ema_n257'].build()
    decay, s = ema_reference(kw['shadow'], kw['param'], kw['step'], kw['ema_decay'])
    wide_ = (decay * kw['shadow'].double() + (1 - decay) * kw['param'].double()).float()
    assert not torch.equal(s, wide_)


# ---- (3) power: one planted fault per family, each on an edge case ------------------------------------------------------------------
FAULTS = [
    ('bn_stats_P257', 'one-pass variance', 'invstd'),
    ('bn_stats_P129', 'one-pass variance', 'invstd'),
    ('bn_stats_last_slice_one_pixel', 'last slice dropped', 'mean'),
    ('bn_stats_P257', 'last slice dropped', 'mean'),
    ('bn_apply_amax_straddle', 'maximum credited to the wrong image', 'amax'),
    ('bn_bwd_amax_straddle', 'maximum credited to the wrong image', 'amax'),
    ('maxpool_bwd_3x3', 'last maximum', 'maxpool3x3s2_bwd'),
    ('maxpool_bwd_1x5', 'last maximum', 'maxpool3x3s2_bwd'),
    ('spp_bwd_3x3_C1', 'last maximum', 'spp_bwd'),
    ('spp_bwd_4x9_C5', 'last maximum', 'spp_bwd'),
    ('bn_bwd_zero_leaky', 'slope 1 at zero', 'dbeta'),
    ('bn_bwd_zero_relu', 'slope 1 at zero', 'bn dx'),
    ('act_bwd_leaky', 'slope 1 at zero', 'act_bwd'),
    ('avgpool2x2_bwd_3x5', 'odd last row filled', 'avgpool2x2_bwd'),
    ('avgpool2x2_bwd_5x2', 'odd last row filled', 'avgpool2x2_bwd'),
    ('upsample2x_bwd_1x1_acc', 'accumulate ignored', 'upsample2x_bwd'),
    ('upsample2x_bwd_3x5_acc', 'accumulate ignored', 'upsample2x_bwd'),
    ('bn_apply_C4', 'channel past the slice', 'outside'),
    ('bn_apply_C1028', 'channel past the slice', 'outside'),
    ('wgrad_1x1map_bf16x3', 'off-centre tap non-zero', 'wgrad'),
    ('wgrad_1x1map_f16x2', 'off-centre tap non-zero', 'wgrad'),
    ('wgrad_1x1map_f16x2', 'off-centre tap a denormal', 'wgrad'),
    ('wgrad_1x1map_bf16x3', 'off-centre tap a denormal', 'wgrad'),
]


@pytest.mark.parametrize('name,fault,what', FAULTS)
def test_planted_fault_fails_the_named_check(name, fault, what):
    rep, _ = run_case(CASES[name], fault)
    assert rep.failures, 'the planted fault (%s) went unnoticed on %s: %s' % (fault, name, rep.report())
    assert any(what in f['what'] for f in rep.failures), rep.report()
    print('%-32s %-38s -> %s' % (name, fault, sorted({f['what'] for f in rep.failures})))


def test_one_pixel_per_channel_hides_the_one_pass_variance():
    """At P = 1 the one- and the two-pass form coincide: the case checks the geometry, not the variance."""
    rep, _ = run_case(CASES['bn_stats_P1'], 'one-pass variance')
    assert not rep.failures


# ---- (4) coverage ---------------------------------------------------------------------------------------------------------------
def test_every_checker_has_a_case_or_is_exempt():
    checkers = {n[4:] for n in vars(lr.Replay) if n.startswith('chk_')}
    used = {c.op for c in CASES.values()}
    assert used <= checkers, sorted(used - checkers)
    missing = sorted(checkers - used - set(tec.EXEMPT))
    assert not missing, 'checkers of the launch replay without an edge case or an exemption: %s' % missing
    assert not (used & set(tec.EXEMPT)) and all(tec.EXEMPT.values())
    assert all(c.why and callable(c.promise) for c in CASES.values())
