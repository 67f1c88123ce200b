"""The training forward and backward of a GroupNorm / AffineChannel / BatchNorm + relu / leaky / mish unit restated with torch on the
CPU (reference model/custom_layers.py:37-62, :118-135, :243-253), in whatever dtype the tensors have: float32 reproduces the g24
golden's float32 rows (tests/test_norm_act_train_host.py), float64 is the answer the GPU tests measure against.  relu / leaky take an
explicit slope mask (True where the slope is 1), so a float64 twin can be locked to the device's own sign pattern -- the practice of
tests/train_parity_util.py.  Plus the g24 golden's access helpers."""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

import norm_act_ref as R

GOLDEN = R.GOLDEN
MISH_PROBE = (-100., -20., -1e-3, 1e-3, 0., 19.99, 20., 20.01, 100.)


def mish_grad(x):
    """n / (n + 2) + x * 4 e (e + 1) / (n + 2)^2 with e = exp(x), n = e (e + 2); x > 20 gives 1 (torch's softplus threshold)."""
    xs = torch.clamp(x, max=20.0)
    e = torch.exp(xs)
    n = e * (e + 2.0)
    d = n + 2.0
    g = n / d + xs * 4.0 * e * (e + 1.0) / (d * d)
    return torch.where(x > 20.0, torch.ones_like(x), g)


def act_grad(z, act, mask=None):
    """act'(z); mask (bool, z's shape): where relu / leaky have slope 1 -- None: z > 0."""
    if act is None:
        return torch.ones_like(z)
    if act == 'mish':
        return mish_grad(z)
    m = (z > 0) if mask is None else mask
    one = torch.ones_like(z)
    return torch.where(m, one, one * (0.0 if act == 'relu' else 0.1))


def _cview(v, x):
    return v.to(x.dtype).view((1, -1) + (1,) * (x.dim() - 2))


def gn_stats(x, groups, eps=1e-5):
    """x NCHW -> xhat (x's shape), rstd [N, groups, 1]: two passes in x's dtype."""
    N = x.shape[0]
    g = x.reshape(N, groups, -1)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return ((g - mean) * rstd).reshape(x.shape), rstd


def gn_fwd_bwd(x, gamma, beta, groups, act, dy, res=None, mask=None, eps=1e-5):
    """GroupNorm(groups)(x) [+ res] -> act, and its backward for the upstream dy.  NCHW.  -> dict(y, dx, dgamma, dbeta, dz)."""
    N = x.shape[0]
    xhat, rstd = gn_stats(x, groups, eps)
    ga, be = _cview(gamma, x), _cview(beta, x)
    z = xhat * ga + be
    if res is not None:
        z = z + res
    dz = dy * act_grad(z, act, mask)
    red = (0,) + tuple(range(2, x.dim()))
    dbeta, dgamma = dz.sum(dim=red), (dz * xhat).sum(dim=red)
    gd = (ga * dz).reshape(N, groups, -1)
    m = gd.shape[2]
    A = gd.sum(dim=2, keepdim=True) / m
    B = (gd * xhat.reshape(N, groups, -1)).sum(dim=2, keepdim=True) / m
    dx = (rstd * (gd - A - xhat.reshape(N, groups, -1) * B)).reshape(x.shape)
    return dict(y=R.act(z, act), dx=dx, dgamma=dgamma, dbeta=dbeta, dz=dz)


def af_fwd_bwd(x, weight, bias, act, dy, res=None, mask=None):
    """act(x * w + b [+ res]) and its backward.  NCHW.  -> dict(y, dx, dgamma (= dw), dbeta (= db), dz)."""
    w, b = _cview(weight, x), _cview(bias, x)
    z = x * w + b
    if res is not None:
        z = z + res
    dz = dy * act_grad(z, act, mask)
    red = (0,) + tuple(range(2, x.dim()))
    return dict(y=R.act(z, act), dx=dz * w, dgamma=(dz * x).sum(dim=red), dbeta=dz.sum(dim=red), dz=dz)


def bn_fwd_bwd(x, gamma, beta, act, dy, mask=None, eps=1e-5):
    """BatchNorm on batch statistics (biased variance) -> act, and its backward.  NCHW."""
    red = (0,) + tuple(range(2, x.dim()))
    cnt = x.numel() // x.shape[1]
    mean = x.mean(dim=red, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=red, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    ga = _cview(gamma, x)
    z = xhat * ga + _cview(beta, x)
    dz = dy * act_grad(z, act, mask)
    dbeta, dgamma = dz.sum(dim=red), (dz * xhat).sum(dim=red)
    dx = ga * rstd * (dz - _cview(dbeta, x) / cnt - xhat * _cview(dgamma, x) / cnt)
    return dict(y=R.act(z, act), dx=dx, dgamma=dgamma, dbeta=dbeta, dz=dz)


class _Slope(torch.autograd.Function):
    """relu / leaky whose backward takes its slopes from an explicit mask (True: slope 1) instead of the sign of its input."""

    @staticmethod
    def forward(ctx, z, mask, slope):
        ctx.save_for_backward(mask)
        ctx.slope = slope
        return F.relu(z) if slope == 0.0 else F.leaky_relu(z, slope)

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        return torch.where(mask, g, g * ctx.slope), None, None


def act_masked(z, name, mask=None):
    """The activation as the reference applies it (tests/norm_act_ref.act); with a mask, relu / leaky differentiate by it."""
    if mask is None or name not in ('relu', 'leaky'):
        return R.act(z, name)
    return _Slope.apply(z, mask, 0.0 if name == 'relu' else 0.1)


def unit_fwd_bwd(meta, sd, x, dy, mask=None):
    """Conv2dUnit in TRAINING mode from its state_dict and its backward for the upstream dy, in x's dtype, with the ATen calls the
    reference's modules make (F.conv2d, F.group_norm, F.batch_norm on batch statistics, the AffineChannel arithmetic, autograd) --
    so float32 is the reference's float32 -- and relu / leaky slopes by `mask` when one is given.
    -> dict(y, dx, grads {state_dict key: gradient})."""
    t = {k: v.detach().to(x.dtype).clone() for k, v in sd.items() if v.is_floating_point()}
    for k, v in t.items():
        if 'running' not in k:
            v.requires_grad_(True)
    xi = x.detach().clone().requires_grad_(True)
    y = F.conv2d(xi, t['conv.weight'], t.get('conv.bias'), stride=meta['stride'], padding=(meta['k'] - 1) // 2)
    if meta['norm'] == 'bn':
        y = F.batch_norm(y, t['bn.running_mean'], t['bn.running_var'], t['bn.weight'], t['bn.bias'], True, 0.1, 1e-5)
    elif meta['norm'] == 'gn':
        y = R.group_norm(y, t['gn.weight'], t['gn.bias'], meta['groups'])
    elif meta['norm'] == 'af':
        y = R.affine_channel(y, t['af.weight'], t['af.bias'])
    y = act_masked(y, meta['act'], mask)
    y.backward(dy.to(x.dtype))
    return dict(y=y.detach(), dx=xi.grad, grads={k: v.grad for k, v in t.items() if v.grad is not None})


def unit_formulas(meta, sd, x, dy, mask=None):
    """The same unit with the norm and activation backward written out (gn_fwd_bwd / af_fwd_bwd / bn_fwd_bwd above: the formulas the
    kernels implement); the convolution by autograd.  -> dict(y, dx, grads)."""
    t = {k: v.detach().to(x.dtype).clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running' not in k}
    xi = x.detach().clone().requires_grad_(True)
    raw = F.conv2d(xi, t['conv.weight'], t.get('conv.bias'), stride=meta['stride'], padding=(meta['k'] - 1) // 2)
    r, n = raw.detach(), meta['norm']
    dy = dy.to(x.dtype)
    if n == 'gn':
        o = gn_fwd_bwd(r, t['gn.weight'].detach(), t['gn.bias'].detach(), meta['groups'], meta['act'], dy, None, mask)
    elif n == 'af':
        o = af_fwd_bwd(r, t['af.weight'].detach(), t['af.bias'].detach(), meta['act'], dy, None, mask)
    else:
        o = bn_fwd_bwd(r, t['bn.weight'].detach(), t['bn.bias'].detach(), meta['act'], dy, mask)
    raw.backward(o['dx'])
    grads = {k: v.grad for k, v in t.items() if k.startswith('conv.')}
    grads[n + '.weight'], grads[n + '.bias'] = o['dgamma'], o['dbeta']
    return dict(y=o['y'], dx=xi.grad, grads=grads)


# ---- the golden -------------------------------------------------------------------------------------------------------------
def load(name='g24_norm_act_train'):
    return R.load(name)


def f32(d, key):
    return torch.from_numpy(d[key])


def f64(d, key):
    """A float64 row: stored as the float32 difference to the float32 row."""
    return torch.from_numpy(d[key]).double() + torch.from_numpy(d[key + '.d64']).double()


def unit_files():
    """The unit cases' arrays: the index file (shared input, count) and its parts, as one dict."""
    idx = load()
    d = {k: idx[k] for k in idx.files}
    for part in range(int(idx['nparts'])):
        f = load('g24_norm_act_train_units%d' % part)
        d.update({k: f[k] for k in f.files})
    return d


def unit_cases():
    """[(prefix, meta dict, x, dy, state_dict)] of the g24 unit cases."""
    d = unit_files()
    out = []
    for i in range(int(d['nunits'])):
        p = 'u%d_' % i
        x = torch.from_numpy(d[p + 'x'] if p + 'x' in d else d['ux'])
        pre = p + 'sd.'
        sd = {k[len(pre):]: torch.from_numpy(v) for k, v in d.items() if k.startswith(pre)}
        out.append((p, ast.literal_eval(str(d[p + 'meta'])), x, torch.from_numpy(d[p + 'dy']), sd))
    return out


def case_id(c):
    return c[0] + (c[1]['special'] or '%s_%s' % (c[1]['norm'], c[1]['act']))


def have(name='g24_norm_act_train'):
    return os.path.exists(os.path.join(GOLDEN, name + '.npz'))


def judge(what, got, ref32, ref64, factor=3.0, floor=1e-6):
    """max |got - f64| <= factor * max |f32 restatement - f64| + floor * max |f64|; prints the figures first.  -> the ratio."""
    r64 = ref64.detach().double()
    e_got = (got.detach().cpu().double() - r64).abs().max().item()
    e_ref = (ref32.detach().double() - r64).abs().max().item()
    bound = factor * e_ref + floor * r64.abs().max().item()
    print('norm_act_train_parity %-40s err %.3e  reference %.3e  bound %.3e  ratio %.3f' % (what, e_got, e_ref, bound, e_got / max(e_ref, 1e-300)))
    assert e_got <= bound, '%s: %.3e against float64, bound %.3e (the float32 restatement: %.3e)' % (what, e_got, bound, e_ref)
    return e_got / max(e_ref, 1e-300)
