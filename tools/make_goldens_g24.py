#!/usr/bin/env python
"""Generate tests/golden/g24_norm_act_train*.npz by running the REFERENCE implementation in training mode: the forward and backward
of GroupNorm / AffineChannel / Mish units, of bottleneck blocks and a head route with GroupNorm, and one training step of three
models (reference model/custom_layers.py:142-253, train.py:416-443 up to all_loss.backward()).

Build-container only, as tools/make_goldens.py (whose import recipe, synthetic inputs and helpers this file uses).  Each fixture
holds inputs, the state_dict, the upstream gradient and the reference's float32 results; the results of a `.double()` copy are kept
as float32 differences to the float32 rows (`<key>.d64`: row64 = row32 + d64, as g23 does).  The fixtures are DATA; no reference
source is stored.  The unit and block cases are split over several files (an index, four unit files, one per block), so each stays a small
committed fixture.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_g24.py

relu / leaky cases: the float32 and the float64 evaluation must agree on the sign of every pre-activation (asserted here), so a
float64 twin locked to the device's slope mask is the golden's float64 row whenever the device agrees with the golden's signs."""
import copy
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG          # noqa: E402  (the reference import recipe runs on import)

Conv2dUnit, gen, save, synth = MG.Conv2dUnit, MG.gen, MG.save, MG.synth
PROBE = (-100., -20., -1e-3, 1e-3, 0., 19.99, 20., 20.01, 100.)


def put(out, key, v32, v64):
    out[key] = v32.detach()
    out[key + '.d64'] = (v64.detach() - v32.detach().double()).float()


def run_train(m, xs, dy):
    """Forward + backward of a reference module in training mode -> (y, [d input], {parameter name: gradient})."""
    m.train()
    m.zero_grad()
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    y = m(*xs)
    y.backward(dy.to(y.dtype))
    return y.detach(), [x.grad for x in xs], {k: q.grad for k, q in m.named_parameters()}


def both(m, xs, dy):
    r32 = run_train(m, xs, dy)
    r64 = run_train(copy.deepcopy(m).double(), [x.double() for x in xs], dy.double())
    return r32, r64


def record(out, p, m, xs, dy, names=('x',), signs=None):
    (y, dxs, gr), (y64, dxs64, gr64) = both(m, xs, dy)
    put(out, p + 'y', y, y64)
    for n, a, b in zip(names, dxs, dxs64):
        put(out, p + 'd' + n, a, b)
    for k in gr:
        put(out, p + 'g.' + k, gr[k], gr64[k])
    for key, v in m.state_dict().items():
        out[p + 'sd.' + key] = v
    out[p + 'dy'] = dy
    if signs:          # every relu / leaky pre-activation has one sign in float32 and float64
        assert bool(((y > 0) == (y64 > 0)).all()), p
    return y


def units():
    g = gen(2424)
    out = {}
    NORM = {'bn': dict(bn=1), 'gn': dict(gn=1), 'af': dict(af=1)}
    # norm, act, cin, cout, k, stride, bias, groups, N, H, W, special   (the g23 table's shapes)
    table = [
        ('gn', None, 32, 32, 3, 1, False, 32, 2, 13, 11, ''),
        ('gn', 'relu', 32, 64, 1, 1, True, 32, 2, 13, 11, ''),
        ('gn', 'leaky', 32, 256, 1, 2, False, 32, 2, 13, 11, ''),
        ('gn', 'mish', 32, 32, 3, 2, True, 4, 2, 13, 11, ''),
        ('gn', 'leaky', 32, 32, 1, 1, True, 32, 2, 1, 1, 'one'),          # H = W = 1, C / groups = 1, m = 1: dx is exactly 0
        ('gn', 'relu', 32, 64, 1, 1, True, 32, 2, 13, 11, 'const'),        # group 0's convolution output is constant: rstd = 1 / sqrt(eps)
        ('gn', 'leaky', 32, 64, 1, 1, True, 32, 2, 13, 11, 'mean'),        # group 1: mean ~1e3, spread ~1e-2
        ('af', 'leaky', 32, 32, 3, 1, True, 32, 2, 13, 11, ''),
        ('af', 'mish', 32, 32, 1, 2, False, 32, 2, 13, 11, ''),
        ('bn', 'mish', 32, 32, 3, 2, False, 32, 2, 13, 11, ''),
        ('af', 'mish', 32, 32, 1, 1, False, 32, 1, 3, 3, 'mish'),          # identity convolution over the Mish probe values: the derivative
    ]
    probe = torch.tensor(PROBE)
    for i, (norm, act, ci, co, k, s, bias, groups, N, H, W, special) in enumerate(table):
        m = Conv2dUnit(ci, co, k, stride=s, bias_attr=bias, groups=groups, act=act, **NORM[norm])
        MG._g23_fill(m, g)
        if (H, W) == (13, 11):
            if 'ux' not in out:
                out['ux'] = torch.randn(N, ci, H, W, generator=g)
                out['ux'][-1] = out['ux'][-1] * 3.0 + 0.5
            x = out['ux']
        else:
            x = torch.randn(N, ci, H, W, generator=g)
            x[-1] = x[-1] * 3.0 + 0.5
        with torch.no_grad():
            if special == 'const':
                m.conv.weight[0:2] = 0.0
                m.conv.bias[0:2] = 0.7
            if special == 'mean':
                m.conv.weight[2:4] *= 1e-2
                m.conv.bias[2:4] = 1000.0
                # float32 keeps 3e-3 of that group's xhat, so no two evaluations agree on the sign of a pre-activation near 0: the
                # group's offset keeps every one of them positive (|xhat| < 4.5 over 286 samples), the slope pattern is not the subject
                m.gn.weight[2:4] = 1.0
                m.gn.bias[2:4] = 6.0
            if special == 'mish':
                m.conv.weight.copy_(torch.eye(ci).view(ci, ci, 1, 1))
                m.af.weight.fill_(1.0)
                m.af.bias.fill_(0.0)
                x = torch.randn(N, ci, H, W, generator=g) * 4.0
                x[0, :, :, :] = probe.view(1, H, W) + 0.0 * x[0]
        Ho, Wo = (H + 2 * ((k - 1) // 2) - k) // s + 1, (W + 2 * ((k - 1) // 2) - k) // s + 1
        dy = torch.randn(N, co, Ho, Wo, generator=g)
        p = 'u%d_' % i
        out[p + 'meta'] = np.array(repr(dict(norm=norm, act=act, cin=ci, cout=co, k=k, stride=s, bias=bias, groups=groups, special=special)))
        if x is not out.get('ux'):
            out[p + 'x'] = x
        record(out, p, m, [x], dy, signs=act in ('relu', 'leaky'))
    # split by unit so that each file stays a small committed fixture: the index file holds the shared input and the count
    save('g24_norm_act_train', nunits=np.array(len(table)), ux=out.pop('ux'), nparts=np.array(4))
    for part in range(4):
        keep = {k: v for k, v in out.items() if int(k[1:k.index('_')]) % 4 == part}
        save('g24_norm_act_train_units%d' % part, **keep)


def blocks():
    from model.resnet_vd import IdentityBlock, ConvBlock
    g = gen(2425)
    out = {}
    m = IdentityBlock(128, [32, 32, 128], 0, 1, 0, False, 0., 1.)
    MG._g23_fill(m, g)
    x = torch.randn(2, 128, 9, 7, generator=g)
    out['b0_x'] = x
    record(out, 'b0_', m, [x], torch.randn(2, 128, 9, 7, generator=g), signs=True)
    m = ConvBlock(64, [32, 32, 128], 0, 1, 0, False, 0., 1., stride=2)
    MG._g23_fill(m, g)
    x = torch.randn(2, 64, 10, 8, generator=g)
    out['b1_x'] = x
    record(out, 'b1_', m, [x], torch.randn(2, 128, 5, 4, generator=g), signs=True)

    class Route(torch.nn.Module):          # a head route: gn conv -> nearest x2 -> concat in front of a backbone map
        def __init__(self):
            super(Route, self).__init__()
            self.conv = Conv2dUnit(64, 32, 1, stride=1, gn=1, act='leaky')
            self.up = torch.nn.Upsample(scale_factor=2, mode='nearest')

        def forward(self, x, skip):
            return torch.cat([self.up(self.conv(x)), skip], dim=1)
    m = Route()
    MG._g23_fill(m, g)
    x, skip = torch.randn(2, 64, 5, 7, generator=g), torch.randn(2, 32, 10, 14, generator=g)
    out['b2_x'], out['b2_skip'] = x, skip
    record(out, 'b2_', m, [x, skip], torch.randn(2, 64, 10, 14, generator=g), names=('x', 'skip'), signs=True)
    for b in range(3):          # one file per block: each a small committed fixture
        save('g24_norm_act_train_block%d' % b, **{k: v for k, v in out.items() if k.startswith('b%d_' % b)})


def model_case(tag, C, S, N, bb_norm, hd_norm, fa):
    cfg = C()
    cfg.backbone['norm_type'], cfg.head['norm_type'] = bb_norm, hd_norm
    cfg.backbone['freeze_at'] = fa
    cfg.head['drop_block'] = False          # DropBlock is pinned elsewhere and independent of the norm: no RNG in this golden
    m = MG.build_ref_train(cfg, 0)
    assert m.training
    gt_bbox, gt_class, gt_score, targets = MG.synth_gt(N, S, cfg, seed=77)
    T = torch.from_numpy
    m64 = copy.deepcopy(m).double()
    # The image seed is the first from 1234 on at which no relu / leaky pre-activation of a TRAINED layer lies within MARGIN of zero:
    # two float32-grade evaluations of the network differ by ~1e-6 there, and one slope that flips moves every gradient upstream of it
    # by 1e-3 .. 1e-2 (measured: one element at |z| = 1e-6 in head.detection_blocks.1.layers.7 of the r50vd case at seed 1234).  What
    # the units below measure is the arithmetic of the norms, not where a kink falls.
    MARGIN = 4e-6

    def near_zero(mm, xin):
        seen, hooks = [], []

        def hook(mod, inp, y):
            if isinstance(y, torch.Tensor) and any(q.requires_grad for q in mod.parameters()):
                z = torch.where(y > 0, y, y * 10.0).abs()          # (leaky: the pre-activation; relu: the positive side)
                seen.append(((z > 0) & (z < MARGIN)).sum().item())
        for mod in mm.modules():
            if type(mod).__name__ in ('Conv2dUnit', 'BasicBlock', 'ConvBlock', 'IdentityBlock'):
                hooks.append(mod.register_forward_hook(hook))
        with torch.no_grad():
            mm.head._get_outputs(mm.backbone(xin))
        for h in hooks:
            h.remove()
        return sum(seen)
    for iseed in range(1234, 1234 + 200):
        x = synth.synth_images(N, S, seed=iseed)
        if near_zero(m, x) == 0 and near_zero(m64, x.double()) == 0:
            break
    else:
        raise SystemExit('%s: no image seed keeps the pre-activations clear of zero' % tag)
    print('   %s: image seed %d' % (tag, iseed))

    def step(mm, dt):
        mm.zero_grad()
        feats = mm.backbone(x.to(dt))
        outs = mm.head._get_outputs(feats)
        for o in outs:
            o.retain_grad()
        hd = mm.head
        losses = hd.yolo_loss(outs, T(gt_bbox).to(dt), T(gt_class), T(gt_score).to(dt), [T(t).to(dt) for t in targets], hd.anchors,
                              hd.anchor_masks, hd.mask_anchors, hd.num_classes)
        total = 0.0
        for k in losses:
            total = total + losses[k]
        total.backward()
        return losses, outs, {k: q.grad for k, q in mm.named_parameters() if q.grad is not None}
    l32, o32, g32 = step(m, torch.float32)
    l64, o64, g64 = step(m64, torch.float64)
    arrs = dict(meta=np.array([S, N, 0, iseed, fa]), norms=np.array([bb_norm, hd_norm]), gt_bbox=gt_bbox, gt_class=gt_class, gt_score=gt_score,
                loss_names=np.array(list(l32.keys())), loss_values=np.array([float(l32[k].detach()) for k in l32], np.float32),
                loss_values64=np.array([float(l64[k].detach()) for k in l64], np.float64))
    for i, t in enumerate(targets):
        arrs['target%d' % i] = t
    for i, (a, b) in enumerate(zip(o32, o64)):
        put(arrs, 'out%d' % i, a, b)
        put(arrs, 'dout%d' % i, a.grad, b.grad)
    names, d32, d64, s32, s64, amax = [], [], [], [], [], []
    for k, q in m.named_parameters():
        stage = int(k[len('backbone.stage')]) if k.startswith('backbone.stage') else 6
        assert (k in g32) == (stage > fa), k
        if k not in g32:
            continue
        a, b = MG.grad_digest(g32[k])
        a6, b6 = MG.grad_digest(g64[k])
        names.append(k); d32.append(a); d64.append(a6); s32.append(np.pad(b, (0, 64 - len(b)))); s64.append(np.pad(b6, (0, 64 - len(b6))))
        amax.append(float(g64[k].abs().max()))
        if k.split('.')[-2] in ('bn', 'gn', 'af'):          # the full gradient of every norm parameter
            put(arrs, 'g.' + k, g32[k], g64[k])
    arrs.update(grad_names=np.array(names), grad_digest=np.stack(d32), grad_digest64=np.stack(d64), grad_samples=np.stack(s32),
                grad_samples64=np.stack(s64), grad_absmax64=np.array(amax))
    print(tag, {k: float(l32[k]) for k in l32}, 'trainable tensors', len(names))
    save('g24_norm_act_train_' + tag, **arrs)


if __name__ == '__main__':
    torch.manual_seed(0)
    if '--models-only' not in sys.argv:
        units()
        blocks()
    model_case('r18vd_96_bn_gn', MG.PPYOLO_r18vd_Config, 96, 2, 'bn', 'gn', 5)
    model_case('r18vd_96_gn_gn', MG.PPYOLO_r18vd_Config, 96, 2, 'gn', 'gn', 4)
    model_case('r50vd_96_af_gn', MG.PPYOLO_2x_Config, 96, 2, 'affine_channel', 'gn', 5)
