"""GroupNorm, AffineChannel and Mish units of the training step: what follows a unit's convolution when
train_plan.norm_form says anything but 'bn' / 'none' -- csrc/norm_act.hip, csrc/norm_act_train.hip behind ops.  Functions over a
TrainStep `ts` (train.py owns the state, the tape and the convolutions).  These ops have no float64 launch replay
(tests/launch_replay.py) yet: tests/test_gpu_norm_act_train.py pins them against the reference's float64 rows instead."""
import torch

from . import ops as K
from . import train_plan as TP
from ._lib import PPYoloHipError, conv_cfg


def norm_units(model):
    """{unit name: (groups, eps)} of the model's GroupNorm units; refuses, by the unit's name, what the GroupNorm / AffineChannel
    training kernels do not implement (train_plan.norm_refusal)."""
    gn = {}
    for name, m in model.named_modules():
        if type(m).__name__ != 'Conv2dUnit':
            continue
        norm = 'gn' if getattr(m, 'gn', None) is not None else ('af' if getattr(m, 'af', None) is not None else None)
        if norm is None:
            continue
        groups = m.gn.num_groups if norm == 'gn' else 1
        why = TP.norm_refusal('%s (%s)' % (name, getattr(m, 'name', '') or 'Conv2dUnit'), norm, m.filters, groups, getattr(m, 'norm_decay', 0.0))
        if why:
            raise PPYoloHipError(why)
        if norm == 'gn':
            if getattr(m, 'bn', None) is not None or getattr(m, 'af', None) is not None:
                raise PPYoloHipError('%s: GroupNorm combined with another norm' % name)
            gn[name] = (int(groups), float(m.gn.eps))
    return gn


def mish_inplace(y):
    K.mish(y.view())


def af_scale_shift(ts, prefix, Kout, conv_bias):
    """A FROZEN AffineChannel over the convolution's bias as the epilogue's (scale, shift): (af.weight, af.bias + conv_bias *
    af.weight) -- the inference path's fold (Conv2dUnit.folded); constant, so made once."""
    key = ('af_fold', prefix)
    if key not in ts._const:
        w, b = ts.sd[prefix + '.af.weight'].detach().float(), ts.sd[prefix + '.af.bias'].detach().float()
        shift = b if conv_bias is None else b + conv_bias.detach().float() * w
        ts._const[key] = (w.contiguous().clone(), shift.contiguous().clone())
    return ts._const[key]


def dest(ts, prefix, shape, trainable, out, coord_out):
    N, Ho, Wo, Kout = shape
    y = out if out is not None else (ts.new_coord(prefix, N, Ho, Wo, Kout) if coord_out else ts.new(N, Ho, Wo, Kout))
    y.req = trainable
    y.amax = None          # nothing here tracks a maximum: the consumers run on the bf16x3 / exact tiles
    return y


def af_folded_unit(ts, prefix, x, xin, ent, stride, pad, act, res, out, coord_out, hw):
    """A frozen AffineChannel unit: scale, shift, shortcut and activation in the convolution's epilogue -- one launch, no tape
    entry (nothing below a frozen unit trains); Mish follows as a launch."""
    cur, krsc = ts.cur, ent['krsc']
    Kout, R, S, Cp = krsc.shape
    if x.req:
        raise PPYoloHipError('%s: a frozen AffineChannel unit above a trainable layer is not implemented' % prefix)
    scale, shift = af_scale_shift(ts, prefix, Kout, ts.sd.get(prefix + '.conv.bias'))
    y = dest(ts, prefix, (xin.N, hw[0], hw[1], Kout), False, out, coord_out)
    conv_act = None if act == 'mish' else act

    def run(cfg_id, splitk):
        K.conv2d_bn_act(xin.view(), krsc, scale, shift, y.view(), stride, pad, conv_act, None if res is None else res.view(), cfg=cfg_id,
                        splitk=splitk, ws=cur.ws, w_x3=None if ts.fp32 else ts._planes(ent))
    key = TP.shape_key('conv', xin.N, xin.H, xin.W, Cp, Kout, R, stride)
    cfg_id, splitk = (-1, 0) if ts.fp32 else TP.train_fwd_cfg(*ts._choose(key, run, R * S * Cp // 32, False), cfg_of=conv_cfg)
    run(cfg_id, splitk)
    if act == 'mish':
        K.mish(y.view())
    cur.flops += 2 * xin.N * hw[0] * hw[1] * Kout * R * S * ent['Cin']
    if ts.acts is not None:
        ts.acts[prefix] = y
    return y


def post_fwd(ts, prefix, nform, raw, trainable, act, res=None, out=None, coord_out=False):
    """What follows the RAW convolution output of a 'gn' / 'af_train' / 'bn_mish' unit (train_plan.norm_form) -> (y, context of
    post_bwd).  The outputs carry no tracked maximum."""
    shape = (raw.N, raw.H, raw.W, raw.C)
    r = None if res is None else res.view()
    if nform == 'gn':
        groups, eps = ts._gn[prefix]
        y = dest(ts, prefix, shape, trainable, out, coord_out)
        mean = torch.empty(raw.N * groups, dtype=torch.float64, device=ts.dev)
        rstd = torch.empty(raw.N * groups, dtype=torch.float32, device=ts.dev)
        K.group_norm_train(raw.view(), ts.param(prefix + '.gn.weight'), ts.param(prefix + '.gn.bias'), groups, eps, y.view(), mean,
                           rstd, act, r, ws=ts.cur.ws)
        return y, ('gn', groups, mean, rstd)
    if nform == 'af_train':
        y = dest(ts, prefix, shape, trainable, out, coord_out)
        K.affine_act(raw.view(), ts.param(prefix + '.af.weight'), ts.param(prefix + '.af.bias'), y.view(), act, r)
        return y, ('af',)
    assert nform == 'bn_mish' and res is None
    y, mean, invstd = ts._bn_fwd(prefix, raw, 0, shape, trainable, None, None, out, coord_out)
    K.mish(y.view())
    return y, ('bn_mish', mean, invstd)


def post_bwd(ts, prefix, nctx, raw, y, dy, act, res=None, mean=None, invstd=None, track=False):
    """Backward of post_fwd -> the gradient of `raw` (no tracked maximum for 'gn' / 'af'); the norm's parameter gradients go
    to ts.G, the shortcut's gradient to res.g.  A unit whose conv bias trains gets that gradient here too."""
    kind = nctx[0]
    if kind == 'bn_mish':
        if len(nctx) == 3:
            mean, invstd = nctx[1], nctx[2]
        # the pre-activation z = gamma * invstd * raw + (beta - mean * gamma * invstd), recomputed from the raw output
        scale = ts.param(prefix + '.bn.weight') * invstd
        shift = ts.param(prefix + '.bn.bias') - mean * scale
        dzm = ts.new(raw.N, raw.H, raw.W, raw.C)
        K.mish_bwd(raw.view(), dy.view(), dzm.view(), scale, shift)
        return ts._bn_bwd(prefix, raw, y, dzm, mean, invstd, None, track)
    d_raw = ts.new(raw.N, raw.H, raw.W, raw.C)
    dz = ts.new(raw.N, raw.H, raw.W, raw.C) if (res is not None and res.req) else None
    r, dzv = None if res is None else res.view(), None if dz is None else dz.view()
    if kind == 'gn':
        _, groups, gmean, rstd = nctx
        K.group_norm_bwd(raw.view(), gmean, rstd, ts.param(prefix + '.gn.weight'), ts.param(prefix + '.gn.bias'), groups, dy.view(),
                         d_raw.view(), act, r, dzv, ts.G[prefix + '.gn.weight'], ts.G[prefix + '.gn.bias'], ws=ts.cur.ws)
    else:
        K.affine_bwd(raw.view(), ts.param(prefix + '.af.weight'), ts.param(prefix + '.af.bias'), dy.view(), d_raw.view(), act, r, dzv,
                     ts.G[prefix + '.af.weight'], ts.G[prefix + '.af.bias'], ws=ts.cur.ws)
    if dz is not None:
        ts.accum(res, dz)
    if prefix + '.conv.bias' in ts.G:
        K.channel_sum(d_raw.view(), ts.G[prefix + '.conv.bias'], ts.cur.ws)
    return d_raw
