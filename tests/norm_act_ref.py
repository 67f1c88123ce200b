"""GroupNorm, AffineChannel and Mish of Conv2dUnit restated with torch functionals (reference model/custom_layers.py:37-62,
:118-135, :243-253), in whatever dtype the tensors have: float32 reproduces the golden's float32 outputs bit for bit
(tests/test_norm_act_host.py), float64 is the exact answer the GPU tests measure against.  Plus the golden's access helpers."""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def mish(x):
    return x * torch.tanh(F.softplus(x))          # (softplus: beta 1, threshold 20 -- x > 20 gives x)


def group_norm(x, gamma, beta, groups, eps=1e-5):
    return F.group_norm(x.contiguous(), groups, gamma, beta, eps)          # (contiguous NCHW: what the reference's convolution hands on)


def group_norm_two_pass(x, gamma, beta, groups, eps=1e-5):
    """The definition, two passes in x's dtype (float64 for an exact answer: ATen's channels-last kernel takes E[x^2] - E[x]^2,
    which loses mean^2 / var * 2^-53 even there)."""
    N, C = x.shape[:2]
    g = x.reshape(N, groups, -1)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(x.shape)
    shape = (1, C) + (1,) * (x.dim() - 2)
    return y * gamma.view(shape) + beta.view(shape)


def affine_channel(x, weight, bias):
    N, C, H, W = x.shape
    out = x.permute(0, 2, 3, 1).reshape(N * H * W, C) * weight + bias
    return out.reshape(N, H, W, C).permute(0, 3, 1, 2)


def act(x, name):
    if name == 'relu':
        return F.relu(x)
    if name == 'leaky':
        return F.leaky_relu(x, 0.1)
    if name == 'mish':
        return mish(x)
    assert name is None
    return x


def unit(meta, sd, x):
    """Conv2dUnit.forward of a plain-convolution unit from its state_dict, in x's dtype."""
    t = {k: v.to(x.dtype) for k, v in sd.items() if v.is_floating_point()}
    y = F.conv2d(x, t['conv.weight'], t.get('conv.bias'), stride=meta['stride'], padding=(meta['k'] - 1) // 2)
    if meta['norm'] == 'bn':
        y = F.batch_norm(y, t['bn.running_mean'], t['bn.running_var'], t['bn.weight'], t['bn.bias'], False, 0.1, 1e-5)
    elif meta['norm'] == 'gn':
        y = group_norm(y, t['gn.weight'], t['gn.bias'], meta['groups'])
    elif meta['norm'] == 'af':
        y = affine_channel(y, t['af.weight'], t['af.bias'])
    return act(y, meta['act'])


# ---- the golden -------------------------------------------------------------------------------------------------------------
_files = {}


def load(name='g23_norm_act'):
    if name not in _files:
        _files[name] = np.load(os.path.join(GOLDEN, name + '.npz'))
    return _files[name]


def y32(d, p):
    return torch.from_numpy(d[p + 'y32'])


def y64(d, p, key='y32', dkey='d64'):
    """The float64 output: stored as the float32 difference to the float32 output."""
    return torch.from_numpy(d[p + key]).double() + torch.from_numpy(d[p + dkey]).double()


def state(d, p):
    pre = p + 'sd.'
    return {k[len(pre):]: torch.from_numpy(d[k]) for k in d.files if k.startswith(pre)}


def unit_cases():
    """[(prefix, meta dict, x, state_dict)] of the unit cases."""
    d = load()
    out = []
    for i in range(int(d['nunits'])):
        p = 'u%d_' % i
        x = torch.from_numpy(d[p + 'x'] if p + 'x' in d.files else d['ux'])
        out.append((p, ast.literal_eval(str(d[p + 'meta'])), x, state(d, p)))
    return out


def surface():
    return ast.literal_eval(str(load()['surface']))


def make_unit(meta, sd=None, **kw):
    """This package's Conv2dUnit of a unit case, loaded with the golden's parameters."""
    from model.custom_layers import Conv2dUnit
    norm = {'bn': dict(bn=1), 'gn': dict(gn=1), 'af': dict(af=1)}[meta['norm']]
    m = Conv2dUnit(meta['cin'], meta['cout'], meta['k'], stride=meta['stride'], bias_attr=meta['bias'], groups=meta['groups'],
                   act=meta['act'], **dict(norm, **kw))
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.eval()


def err_ratio(got, d, p, key='y32', dkey='d64'):
    """(error of `got` against the float64 output, error of the reference's own float32 output against it), both max abs."""
    ref64 = y64(d, p, key, dkey)
    e_got = (got.detach().cpu().double() - ref64).abs().max().item()
    e_ref = torch.from_numpy(d[p + dkey]).double().abs().max().item()
    return e_got, e_ref
