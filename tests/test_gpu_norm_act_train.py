"""GroupNorm / AffineChannel / Mish in the training step on the MI355X: the backward kernels called directly, unit and block cases
through TrainStep.conv_unit and the tape, three models through the whole step, and the plumbing around the new parameters.

Bounds.  A kernel result is judged against the float64 restatement (tests/norm_act_train_ref.py) on the same slope mask:
max |hip - f64| <= K_GN * max |f32 restatement - f64| + 1e-6 * max |f64| -- K_GN = 3 is the factor of tests/test_gpu_norm_act.py and
the training suite's "3 x the reference's own error" (tests/test_gpu_train_step.py); the floor has the form of that file's
`3.0 * e_ref + 1e-6`.  Every figure is printed before it is asserted (profiles/norm_act_train_parity.txt holds the worst per family)."""
import numpy as np
import pytest
import torch

import norm_act_ref as R
import norm_act_train_ref as T
from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from ppyolo_hip import synth

pytestmark = pytest.mark.gpu

K_GN = 3.0


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _view(t_nhwc, pad, off, fill=7.25):
    """The tensor as a channel slice [off, off + C) of a buffer `pad` channels wider."""
    from ppyolo_hip import ops as K
    N, H, W, C = t_nhwc.shape
    buf = torch.full((N, H, W, C + pad), fill)
    buf[..., off:off + C] = t_nhwc
    return K.View(buf.cuda(), off, C)


def _slope_mask(y, act):
    return (y > 0) if act in ('relu', 'leaky') else None


# ---- the kernels, called directly -----------------------------------------------------------------------------------------------
GN_SHAPES = [  # N, H, W, C, groups, act, residual, ld > C
    (2, 13, 11, 64, 32, 'leaky', False, False),         # base case
    (2, 13, 11, 64, 32, 'relu', True, False),           # ... with a residual: dz comes back
    (2, 13, 11, 64, 32, 'mish', False, True),           # ... with ld > C on x, dy and dx
    (2, 1, 1, 32, 32, 'leaky', False, False),           # m = 1: dx is exactly 0
    (1, 3, 4, 32, 4, None, False, False),               # few groups
    (2, 19, 19, 256, 32, 'leaky', False, False),        # several pixel chunks
    (1, 3, 3, 2048, 32, 'relu', False, False),          # channel slabs
]


def _gn_case(N, H, W, C, groups, act, with_res, wide, seed=0):
    from ppyolo_hip import ops as K
    gen = torch.Generator().manual_seed(2400 + C + H + seed)
    x = torch.randn(N, C, H, W, generator=gen)
    x[-1] = x[-1] * 2.5 - 0.75
    dy = torch.randn(N, C, H, W, generator=gen)
    res = torch.randn(N, C, H, W, generator=gen) if with_res else None
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    pad, off = (24, 8) if wide else (0, 0)
    xv, dyv = _view(nhwc(x), pad, off), _view(nhwc(dy), pad, off)
    rv = _view(nhwc(res), 8, 4) if with_res else None
    yv, dxv = _view(torch.zeros(N, H, W, C), 0, 0), _view(torch.zeros(N, H, W, C), pad, off)
    dzv = _view(torch.zeros(N, H, W, C), 0, 0) if with_res else None
    mean = torch.empty(N * groups, dtype=torch.float64, device='cuda')
    rstd = torch.empty(N * groups, dtype=torch.float32, device='cuda')
    g, b = gamma.cuda(), beta.cuda()
    K.group_norm_train(xv, g, b, groups, 1e-5, yv, mean, rstd, act, rv)
    return dict(x=x, dy=dy, res=res, gamma=gamma, beta=beta, xv=xv, dyv=dyv, rv=rv, yv=yv, dxv=dxv, dzv=dzv, mean=mean, rstd=rstd, g=g, b=b)


def _gn_bwd(c, groups, act, train=True):
    from ppyolo_hip import ops as K
    C = c['gamma'].numel()
    dg = torch.full((C,), -5.5, device='cuda') if train else None
    db = torch.full((C,), -5.5, device='cuda') if train else None
    K.group_norm_bwd(c['xv'], c['mean'], c['rstd'], c['g'], c['b'], groups, c['dyv'], c['dxv'], act, c['rv'], c['dzv'], dg, db)
    torch.cuda.synchronize()
    return nchw(c['dxv'].dense().cpu()), dg, db, (nchw(c['dzv'].dense().cpu()) if c['dzv'] is not None else None)


@pytest.mark.parametrize('N,H,W,C,groups,act,with_res,wide', GN_SHAPES)
def test_group_norm_backward_kernel(N, H, W, C, groups, act, with_res, wide):
    from ppyolo_hip import ops as K
    c = _gn_case(N, H, W, C, groups, act, with_res, wide)
    # the training forward is the inference forward, bit for bit
    y2 = _view(torch.zeros(N, H, W, C), 0, 0)
    K.group_norm(c['xv'], c['g'], c['b'], groups, 1e-5, y2, act, c['rv'])
    torch.cuda.synchronize()
    y = nchw(c['yv'].dense().cpu())
    assert torch.equal(y, nchw(y2.dense().cpu()))
    dx, dg, db, dz = _gn_bwd(c, groups, act)
    mask = _slope_mask(y, act)
    r32 = T.gn_fwd_bwd(c['x'], c['gamma'], c['beta'], groups, act, c['dy'], c['res'], mask)
    r64 = T.gn_fwd_bwd(c['x'].double(), c['gamma'].double(), c['beta'].double(), groups, act, c['dy'].double(),
                       None if c['res'] is None else c['res'].double(), mask)
    if mask is not None:
        print('slope mask: %d elements differ from the float64 sign pattern' % int((mask != (r64['y'] > 0)).sum()))
    tag = 'gn %s' % ((N, H, W, C, groups, act),)
    T.judge(tag + ' dx', dx, r32['dx'], r64['dx'], K_GN)
    T.judge(tag + ' dgamma', dg.cpu(), r32['dgamma'], r64['dgamma'], K_GN)
    T.judge(tag + ' dbeta', db.cpu(), r32['dbeta'], r64['dbeta'], K_GN)
    if with_res:
        T.judge(tag + ' dz', dz, r32['dz'], r64['dz'], K_GN)
    if wide:          # nothing outside the slice
        full = c['dxv'].t.cpu()
        assert bool((full[..., :8] == 7.25).all()) and bool((full[..., 8 + C:] == 7.25).all())
    if H * W * C // groups == 1:
        assert torch.equal(dx, torch.zeros_like(dx)), 'm = 1: dx must be exactly zero'
    # two runs are bit-identical
    dx2, dg2, db2, _ = _gn_bwd(c, groups, act)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)
    # frozen: dgamma / dbeta are not touched, dx is the same
    from ppyolo_hip._lib import lib, NORM_ACT
    ws = torch.empty(int(lib().ppy_group_norm_bwd_workspace_bytes(N, H, W, C, groups)) // 4 + 2, device='cuda')
    keep_g, keep_b = torch.full((C,), 3.5, device='cuda'), torch.full((C,), 4.5, device='cuda')
    c['dxv'].t.fill_(7.25)
    rc = lib().ppy_group_norm_bwd_f32(c['xv'].ptr, c['xv'].ld, c['mean'].data_ptr(), c['rstd'].data_ptr(), c['g'].data_ptr(), c['b'].data_ptr(),
                                      groups, NORM_ACT[act], None if c['rv'] is None else c['rv'].ptr, 0 if c['rv'] is None else c['rv'].ld,
                                      c['dyv'].ptr, c['dyv'].ld, c['dxv'].ptr, c['dxv'].ld, None, 0, keep_g.data_ptr(), keep_b.data_ptr(), 0,
                                      N, H, W, C, ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((keep_g == 3.5).all()) and bool((keep_b == 4.5).all())
    assert torch.equal(nchw(c['dxv'].dense().cpu()), dx)


def test_group_norm_backward_rejects_bad_arguments():
    from ppyolo_hip import ops as K
    from ppyolo_hip._lib import lib
    c = _gn_case(1, 4, 4, 64, 32, None, False, False)
    args = lambda groups, C, ws, nbytes, ld=64, x_ld=None: lib().ppy_group_norm_bwd_f32(
        c['xv'].ptr, x_ld or ld, c['mean'].data_ptr(), c['rstd'].data_ptr(), c['g'].data_ptr(), c['b'].data_ptr(), groups, 0, None, 0,
        c['dyv'].ptr, ld, c['dxv'].ptr, ld, None, 0, None, None, 0, 1, 4, 4, C, ws, nbytes, None)
    ws = torch.empty(1 << 16, device='cuda')
    assert args(24, 64, ws.data_ptr(), ws.numel() * 4) == -1                # PPY_ERR_BAD_ARG: 64 % 24
    assert args(32, 64, ws.data_ptr(), ws.numel() * 4, x_ld=60) == -1       # ld < C
    assert args(32, 64, ws.data_ptr(), 64) == -3                            # PPY_ERR_WORKSPACE
    assert args(32, 64, None, 0) == -3
    assert args(32, 4096, ws.data_ptr(), ws.numel() * 4, ld=4096) == -2   # PPY_ERR_UNSUPPORTED: C > 2048
    assert lib().ppy_group_norm_bwd_f32(c['xv'].ptr, 64, c['mean'].data_ptr(), c['rstd'].data_ptr(), c['g'].data_ptr(), c['b'].data_ptr(), 32,
                                        0, None, 0, c['dyv'].ptr, 64, c['dxv'].ptr, 64, None, 0, None, None, 1, 1, 4, 4, 64, ws.data_ptr(),
                                        ws.numel() * 4, None) == -1          # param_grads without dgamma / dbeta
    assert lib().ppy_affine_bwd_f32(c['xv'].ptr, 64, c['g'].data_ptr(), c['b'].data_ptr(), 0, None, 0, c['dyv'].ptr, 64, c['dxv'].ptr, 64,
                                    None, 0, c['g'].data_ptr(), c['b'].data_ptr(), 1, 1, 4, 4, 64, None, 0, None) == -3
    assert lib().ppy_mish_bwd_f32(c['xv'].ptr, 62, None, None, c['dyv'].ptr, 64, c['dxv'].ptr, 64, 1, 4, 4, 64, None) == -1
    torch.cuda.synchronize()


def test_mish_backward_kernel(capsys):
    """Within 4 ulp of the float64 formula rounded to float32, on the probe row and on random values (scale 1, shift 0: the
    pre-activation is the input itself).  An ulp is that of the reference value, or of the smallest normal float32 for references
    below it (the device may flush subnormals to zero).  With a scale and a shift the float32 pre-activation z = x * scale + shift
    carries up to two roundings of its own, 2^-23 |z| at the most with |x * scale| <= ~2 |z| here, which |mish''| < 1.2 hands on."""
    from ppyolo_hip import ops as K
    gen = torch.Generator().manual_seed(24)
    N, H, W, C = 2, 9, 9, 260
    x = torch.randn(N, H, W, C, generator=gen) * 8.0
    probe = torch.tensor(T.MISH_PROBE)
    x[0, 0, 0, :probe.numel()] = probe
    x[0, 0, 1, :64] = -1.1924 + torch.linspace(-1e-3, 1e-3, 64)          # around the zero of mish'
    dy = torch.ones(N, H, W, C)
    xv, dyv, dxv = _view(x, 12, 8), _view(dy, 0, 0), _view(torch.zeros(N, H, W, C), 20, 16)
    K.mish_bwd(xv, dyv, dxv)
    torch.cuda.synchronize()
    got = dxv.dense().cpu()
    ref = T.mish_grad(x.double()).float()

    def ulp_of(r):
        return torch.maximum(r.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2().double() * 2.0 ** -23
    worst = ((got.double() - ref.double()).abs() / ulp_of(ref)).max().item()
    with capsys.disabled():
        print('\nmish_bwd: worst %.2f ulp over %d values (probe row: %s)' % (worst, got.numel(), got[0, 0, 0, :probe.numel()].tolist()))
    assert worst <= 4.0, 'mish backward: %.2f ulp' % worst
    at = {v: i for i, v in enumerate(T.MISH_PROBE)}
    assert [got[0, 0, 0, at[v]].item() for v in (20.01, 100.)] == [1.0, 1.0], 'x > 20 gives 1'
    full = dxv.t.cpu()
    assert bool((full[..., :16] == 7.25).all()) and bool((full[..., 16 + C:] == 7.25).all())
    # with the norm's scale and shift, and an upstream gradient
    scale, shift = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    dy = torch.randn(N, H, W, C, generator=gen)
    dyv = _view(dy, 0, 0)
    K.mish_bwd(xv, dyv, dxv, scale.cuda(), shift.cuda())
    torch.cuda.synchronize()
    got = dxv.dense().cpu().double()
    z = x.double() * scale.double() + shift.double()
    ref = dy.double() * T.mish_grad(z)
    bound = 5.0 * ulp_of(ref.float()) + dy.double().abs() * 1.2 * 2.0 ** -23 * ((x.double() * scale.double()).abs() + z.abs())
    assert bool(((got - ref).abs() <= bound).all()), ((got - ref).abs() / bound).max().item()


AF_SHAPES = [(2, 13, 11, 64, 'leaky', False, False), (2, 13, 11, 64, 'mish', True, True), (2, 19, 19, 256, 'relu', True, False),
             (1, 3, 3, 2048, None, False, False), (3, 40, 40, 32, 'leaky', False, False)]


@pytest.mark.parametrize('N,H,W,C,act,with_res,wide', AF_SHAPES)
def test_affine_channel_backward_kernel(N, H, W, C, act, with_res, wide):
    from ppyolo_hip import ops as K
    gen = torch.Generator().manual_seed(2450 + C + H)
    x = torch.randn(N, C, H, W, generator=gen) * 1.5 + 0.2
    dy = torch.randn(N, C, H, W, generator=gen)
    res = torch.randn(N, C, H, W, generator=gen) if with_res else None
    w, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    pad, off = (24, 8) if wide else (0, 0)
    xv, dyv, dxv = _view(nhwc(x), pad, off), _view(nhwc(dy), pad, off), _view(torch.zeros(N, H, W, C), pad, off)
    rv = _view(nhwc(res), 8, 4) if with_res else None
    dzv = _view(torch.zeros(N, H, W, C), 0, 0) if with_res else None
    yv = _view(torch.zeros(N, H, W, C), 0, 0)
    wc, bc = w.cuda(), b.cuda()
    K.affine_act(xv, wc, bc, yv, act, rv)
    torch.cuda.synchronize()
    y = nchw(yv.dense().cpu())
    mask = _slope_mask(y, act)
    r32 = T.af_fwd_bwd(x, w, b, act, dy, res, mask)
    r64 = T.af_fwd_bwd(x.double(), w.double(), b.double(), act, dy.double(), None if res is None else res.double(), mask)
    tag = 'af %s' % ((N, H, W, C, act),)
    T.judge(tag + ' y', y, r32['y'], r64['y'], K_GN)

    def run(train):
        dw = torch.full((C,), -5.5, device='cuda') if train else None
        db = torch.full((C,), -5.5, device='cuda') if train else None
        K.affine_bwd(xv, wc, bc, dyv, dxv, act, rv, dzv, dw, db)
        torch.cuda.synchronize()
        return nchw(dxv.dense().cpu()), dw, db
    dx, dw, db = run(True)
    if mask is not None:
        print('slope mask: %d elements differ from the float64 sign pattern' % int((mask != (r64['y'] > 0)).sum()))
    T.judge(tag + ' dx', dx, r32['dx'], r64['dx'], K_GN)
    T.judge(tag + ' dweight', dw.cpu(), r32['dgamma'], r64['dgamma'], K_GN)
    T.judge(tag + ' dbias', db.cpu(), r32['dbeta'], r64['dbeta'], K_GN)
    if with_res:
        T.judge(tag + ' dz', nchw(dzv.dense().cpu()), r32['dz'], r64['dz'], K_GN)
    if wide:
        full = dxv.t.cpu()
        assert bool((full[..., :8] == 7.25).all()) and bool((full[..., 8 + C:] == 7.25).all())
    dx2, dw2, db2 = run(True)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)          # bit-identical from run to run
    dx3, none_w, none_b = run(False)                                                     # frozen: no parameter gradient, the same dx
    assert none_w is None and none_b is None and torch.equal(dx3, dx)


# ---- unit and block cases of g24 through TrainStep.conv_unit and the tape -------------------------------------------------------
class _UnitCfg(object):
    """What TrainStep reads from a configuration when it runs single layers."""
    backbone = dict(freeze_at=5)
    head = {}
    optimizerBuilder = dict(optimizer=dict(momentum=0.9), regularizer=dict(factor=0.0))
    use_ema = False


class _Wrap(torch.nn.Module):
    def __init__(self, **mods):
        super(_Wrap, self).__init__()
        for k, m in mods.items():
            setattr(self, k, m)


@torch.no_grad()
def _tape(ts, y, dy):
    from ppyolo_hip.train import Act
    ts._alloc_flat()
    y.g = Act(nhwc(dy).cuda())
    for fn in reversed(ts.cur.tape):
        fn()
    ts._join_wgrad()
    torch.cuda.synchronize()
    return ts.grads()


def _judge_rows(tag, d, p, got, family):
    """got: {golden key below p: tensor}, each against the golden's float64 row with the reference's own float32 row as yardstick."""
    worst = 0.0
    for key, t in got.items():
        worst = max(worst, T.judge('%s %s%s' % (family, tag, key), t, T.f32(d, p + key), T.f64(d, p + key), K_GN))
    return worst


UNITS = T.unit_cases()


@pytest.mark.parametrize('case', UNITS, ids=[T.case_id(c) for c in UNITS])
def test_unit_cases_through_the_training_step(case):
    from ppyolo_hip.train import Act, TrainStep
    p, meta, x, dy, sd = case
    d = T.unit_files()
    wrap = _Wrap(u=R.make_unit(meta, sd)).cuda()
    ts = TrainStep(wrap, _UnitCfg())
    xa = Act(nhwc(x).cuda(), req=True)
    with torch.no_grad():
        y = ts.conv_unit('u', xa, meta['stride'], meta['act'])
    assert y.amax is None or meta['norm'] == 'bn'          # GroupNorm / AffineChannel outputs carry no tracked maximum
    grads = _tape(ts, y, dy)
    yd = y.dense_nchw().cpu()
    if meta['act'] in ('relu', 'leaky'):
        # the float64 twin is the restatement locked to the device's mask; where the device's signs are the golden's, that twin is
        # the golden's float64 row (tests/test_norm_act_train_host.py)
        differ = int(((yd > 0) != (T.f32(d, p + 'y') > 0)).sum())
        print('%s: %d elements whose golden sign differs' % (T.case_id(case), differ))
        assert differ == 0
    got = {'y': yd, 'dx': xa.g.dense_nchw().cpu()}
    got.update({'g.' + k[2:]: v.cpu() for k, v in grads.items()})
    assert sorted(got) == sorted(k[len(p):] for k in d if k.startswith(p) and not k.endswith('.d64') and k[len(p):].split('.')[0] in ('y', 'dx', 'g'))
    _judge_rows(T.case_id(case) + ' ', d, p, got, 'unit')
    if meta['special'] == 'one':
        assert float(got['dx'].abs().max()) == 0.0 and float(got['g.conv.weight'].abs().max()) == 0.0


@pytest.mark.parametrize('which', ['b0_identity', 'b1_convblock'])
def test_bottleneck_blocks_with_group_norm_train(which):
    """relu(gn(conv3) + shortcut): the residual is added after the norm, and its gradient is the GroupNorm backward's dz."""
    from model.resnet_vd import ConvBlock, IdentityBlock
    from ppyolo_hip.train import Act, TrainStep
    p = which[:3]
    d = R.load('g24_norm_act_train_block%s' % p[1])
    blk = (IdentityBlock(128, [32, 32, 128], 0, 1, 0, False, 0., 1.) if p == 'b0_' else ConvBlock(64, [32, 32, 128], 0, 1, 0, False, 0., 1., stride=2))
    blk.load_state_dict(R.state(d, p), strict=True)
    ts = TrainStep(_Wrap(blk=blk).cuda(), _UnitCfg())
    xa = Act(nhwc(torch.from_numpy(d[p + 'x'])).cuda(), req=True)
    with torch.no_grad():
        y = ts._bottleneck('blk', xa, 1 if p == 'b0_' else 2, p == 'b1_', False)
    grads = _tape(ts, y, torch.from_numpy(d[p + 'dy']))
    yd = y.dense_nchw().cpu()
    differ = int(((yd > 0) != (T.f32(d, p + 'y') > 0)).sum())
    print('%s: %d output elements whose golden sign differs' % (which, differ))
    assert differ == 0
    got = {'y': yd, 'dx': xa.g.dense_nchw().cpu()}
    got.update({'g.' + k[4:]: v.cpu() for k, v in grads.items()})
    assert sorted(got) == sorted(k[len(p):] for k in d.files if not k.endswith('.d64') and k[len(p):].split('.')[0] in ('y', 'dx', 'g'))
    _judge_rows(which + ' ', d, p, got, 'block')


@torch.no_grad()
def test_head_route_with_group_norm_train():
    """gn conv -> nearest x2 -> concat, as TrainStep.head builds a route; the upsample's backward feeds the GroupNorm backward."""
    from ppyolo_hip import ops as K
    from ppyolo_hip.train import Act, TrainStep
    d = R.load('g24_norm_act_train_block2')
    p = 'b2_'
    meta = dict(norm='gn', act='leaky', cin=64, cout=32, k=1, stride=1, bias=False, groups=32)
    sd = {k[len('conv.'):]: v for k, v in R.state(d, p).items()}
    ts = TrainStep(_Wrap(conv=R.make_unit(meta, sd)).cuda(), _UnitCfg())
    x, skip, dy = (torch.from_numpy(d[p + k]) for k in ('x', 'skip', 'dy'))
    xa = Act(nhwc(x).cuda(), req=True)
    route = ts.conv_unit('conv', xa, 1, 'leaky')
    wide = ts.new(2, 10, 14, 64, req=True)
    K.upsample2x(route.view(), wide.slice(0, 32).view())
    wide.t[..., 32:] = nhwc(skip).cuda()
    ts._alloc_flat()
    wide.g = Act(nhwc(dy).cuda())
    g = ts.new(2, 5, 7, 32)
    K.upsample2x_bwd(wide.g.slice(0, 32).view(), g.view())
    route.g = g
    for fn in reversed(ts.cur.tape):
        fn()
    ts._join_wgrad()
    torch.cuda.synchronize()
    yd = wide.dense_nchw().cpu()
    differ = int(((yd[:, :32] > 0) != (T.f32(d, p + 'y')[:, :32] > 0)).sum())
    print('route: %d elements whose golden sign differs' % differ)
    assert differ == 0
    got = {'y': yd, 'dx': xa.g.dense_nchw().cpu(), 'dskip': nchw(wide.g.t[..., 32:].cpu())}
    got.update({'g.' + k: v.cpu() for k, v in ts.grads().items()})
    _judge_rows('route ', d, p, got, 'block')


# ---- models ---------------------------------------------------------------------------------------------------------------------
MODELS = [('r18vd_96_bn_gn', PPYOLO_r18vd_Config, 'bn', 'gn', 5), ('r18vd_96_gn_gn', PPYOLO_r18vd_Config, 'gn', 'gn', 4),
          ('r50vd_96_af_gn', PPYOLO_2x_Config, 'affine_channel', 'gn', 5)]


def _model_cfg(cfgc, bb, hd, fa):
    cfg = cfgc()
    cfg.backbone['norm_type'], cfg.head['norm_type'] = bb, hd
    cfg.backbone['freeze_at'] = fa
    cfg.head['drop_block'] = False          # (DropBlock is pinned elsewhere and independent of the norm)
    return cfg


def relmax(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize('tag,cfgc,bb,hd,fa', MODELS)
def test_models_train_one_step_against_the_reference(tag, cfgc, bb, hd, fa, capsys):
    """Forms and numbers of tests/test_gpu_train_step.py: losses within 2e-3, head outputs within 1e-2 of their maximum, gradient
    digests with median relative error <= 1e-3 and maximum <= 3e-2; the loss gradient is the reference's (the loss has kinks: that
    file's reasoning).  Plus: the trained tensors are the golden's, and every norm parameter's full gradient within factor 3 of float64."""
    from ppyolo_hip.train import TrainStep
    d = R.load('g24_norm_act_train_' + tag)
    S, N, seed, iseed, gfa = [int(v) for v in d['meta']]
    assert gfa == fa
    cfg = _model_cfg(cfgc, bb, hd, fa)
    model, _ = build_model(cfg, seed, 'cuda')
    ts = TrainStep(model, cfg)          # (the parent commit raised here: GroupNorm / AffineChannel were refused by name)
    x = synth.synth_images(N, S, seed=iseed).cuda()
    n_lvl = len(cfg.head['anchor_masks'])
    targets = [torch.from_numpy(d['target%d' % i]).cuda() for i in range(n_lvl)]
    douts = [T.f32(d, 'dout%d' % i) for i in range(n_lvl)]
    loss6 = ts.forward_backward(x, torch.from_numpy(d['gt_bbox']).cuda(), targets, inject_douts=douts)
    torch.cuda.synchronize()
    lines = []
    names = ['loss_xy', 'loss_wh', 'loss_obj', 'loss_cls', 'loss_iou', 'loss_iou_aware']
    for nme, want in zip([str(v) for v in d['loss_names']], d['loss_values']):
        got = float(loss6[names.index(nme)])
        lines.append('%s %s: %.6f, reference %.6f' % (tag, nme, got, float(want)))
        assert abs(got - float(want)) <= 2e-3 * abs(float(want)), lines[-1]
    for i, o in enumerate(ts.outs):
        e = relmax(o.dense_nchw(), T.f32(d, 'out%d' % i))
        own = relmax(T.f64(d, 'out%d' % i), T.f32(d, 'out%d' % i))
        lines.append('%s head output %d: max error %.3e of the maximum (the reference\'s float32 against its float64: %.3e)' % (tag, i, e, own))
        assert e <= 1e-2, lines[-1]
    grads = ts.grads()
    gnames = [str(v) for v in d['grad_names']]
    assert sorted(grads) == sorted(gnames)
    worst = {}
    for j, k in enumerate(gnames):
        g = grads[k].detach().double().reshape(-1).cpu()
        step = max(1, g.numel() // 64)
        smp = g[::step][:64]
        ref = torch.from_numpy(d['grad_samples'][j][:smp.numel()]).double()
        l2 = g.pow(2).sum().sqrt().item()
        worst[k] = max((smp - ref).abs().max().item() / max(float(d['grad_absmax64'][j]), 1e-30),
                       abs(l2 - float(d['grad_digest'][j][2])) / max(float(d['grad_digest'][j][2]), 1e-30))
    med, mx = float(np.median(list(worst.values()))), max(worst.values())
    lines.append('%s gradient digests over %d tensors: median relative error %.3e, maximum %.3e' % (tag, len(worst), med, mx))
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    assert med <= 1e-3 and mx <= 3e-2, {k: v for k, v in worst.items() if v > 2e-3}
    ratios = {}
    for k in gnames:
        if k.split('.')[-2] in ('bn', 'gn', 'af'):
            ratios[k] = T.judge('model %s %s' % (tag, k), grads[k].cpu(), T.f32(d, 'g.' + k), T.f64(d, 'g.' + k), K_GN)
    assert ratios


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def _gn_head_setup(bb='bn', fa=5, train_model=False, seed=0):
    from conftest import build_train_model
    d = R.load('g24_norm_act_train_r18vd_96_bn_gn')
    cfg = _model_cfg(PPYOLO_r18vd_Config, bb, 'gn', fa)
    model = build_train_model(cfg, seed, 'cuda') if train_model else build_model(cfg, seed, 'cuda')[0]
    x = synth.synth_images(2, 96, seed=1234).cuda()
    gt = torch.from_numpy(d['gt_bbox']).cuda()
    targets = [torch.from_numpy(d['target%d' % i]).cuda() for i in range(len(cfg.head['anchor_masks']))]
    return cfg, model, x, gt, targets


def test_three_steps_move_the_group_norm_parameters():
    """SGD without weight decay on the norm parameters (p - lr * g after the first step), the EMA shadow of model/EMA.py, a frozen
    AffineChannel backbone left bit for bit, sync_to_model writing the gn.* keys back."""
    from ppyolo_hip.train import TrainStep
    cfg, model, x, gt, targets = _gn_head_setup(bb='affine_channel')
    cfg.use_ema = True
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    ts = TrainStep(model, cfg)
    key = [k for k in ts.train_keys if k.endswith('.gn.weight')][0]
    lr = 0.002
    losses = [ts.step(x, gt, targets, lr)]
    ts._await_params()
    torch.cuda.synchronize()
    assert ts.layout[key][0] >= ts.n_decay and ts.layout[key[:-6] + 'bias'][0] >= ts.n_decay
    g, p1 = ts.G[key].clone(), ts.P[key].clone()
    assert float(g.abs().max()) > 0
    want = sd0[key].double() - lr * g.double()
    assert (p1.double() - want).abs().max().item() <= 2.0 ** -22 * want.abs().max().item()          # first step: v = g, no decay
    d0 = min(ts.ema_decay, 1.0 / 10.0)
    o, n, _ = ts.layout[key]
    shadow = ts.sflat[o:o + n]
    ema = d0 * sd0[key].double() + (1.0 - d0) * p1.double()
    assert (shadow.double() - ema).abs().max().item() <= 2.0 ** -22 * ema.abs().max().item()
    for _ in range(2):
        losses.append(ts.step(x, gt, targets, lr))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(l).all()) for l in losses)
    ts.sync_to_model()
    sd = model.state_dict()
    for k in ts.train_keys:
        if '.gn.' in k:
            assert not torch.equal(sd[k], sd0[k]), k
            assert torch.equal(sd[k], ts.P[k].view(sd[k].shape)), k
    frozen = [k for k in sd if k.startswith('backbone.') and '.af.' in k]
    assert frozen and all(torch.equal(sd[k], sd0[k]) for k in frozen)
    ts.sync_to_model(ema=True)
    assert torch.equal(model.state_dict()[key], ts.sflat[o:o + n])


def test_loss_dict_hands_torch_the_group_norm_gradients():
    from ppyolo_hip.train import loss_dict
    cfg, model, x, gt, targets = _gn_head_setup(train_model=True)
    losses = loss_dict(model, x, gt, targets)
    sum(losses.values()).backward()
    ts = model._train_bridge
    grads = ts.grads()
    seen = 0
    for k, q in model.named_parameters():
        if q.requires_grad:
            assert q.grad is not None and torch.equal(q.grad, grads[k]), k
            seen += '.gn.' in k
        else:
            assert q.grad is None, k
    assert seen > 0 and all(bool(torch.isfinite(v).all()) for v in losses.values())


def test_prefetched_group_norm_backbone_is_the_plain_loop():
    """prefetch_backbone on a frozen gn backbone (no batch statistics, no counters to bump): the plain loop's results bit for bit."""
    from ppyolo_hip.train import TrainStep
    runs = []
    for prefetch in (False, True):
        cfg, model, x, gt, targets = _gn_head_setup(bb='gn')
        x2 = synth.synth_images(2, 96, seed=99).cuda()
        ts = TrainStep(model, cfg)
        a = ts.step(x, gt, targets, 0.002, next_x=x2 if prefetch else None).clone()
        assert (ts._pref is not None) == prefetch
        b = ts.step(x2, gt, targets, 0.002).clone()
        ts._await_params()
        torch.cuda.synchronize()
        runs.append((a, b, ts.gflat.clone(), ts.pflat.clone()))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
