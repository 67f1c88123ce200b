"""Inputs of ppy_dcnv2_backward_f32 (csrc/dcn.hip) at the positions random offsets never reach, and their oracle  -- device-free
TEST INFRASTRUCTURE (tests/test_dcn_cases.py checks the builders on the CPU, tests/test_gpu_dcn_edges.py runs the kernels).

The reference initialises conv_offset to zero (model/custom_layers.py:510-511): a from-scratch training starts with every
offset exactly 0, every sampling position an integer and the border taps exactly ON the clamp bounds [0, H+2p-1], where
torch.clamp's backward passes the gradient.  Pad 1 throughout; shapes are (N, H, W, C, K, stride).

Oracle: oracle/ppyolo_oracle.dcnv2_sample on leaf tensors x, offset, mask LOGITS (through torch.sigmoid), contracted with w,
y.backward(dy): d x (sampling path only = what the entry point returns), d offset_mask, d w.  float32 reproduces the
reference's arithmetic (the image index folded into the row coordinate); float64 is the accuracy reference.
"""
import functools

import torch

from oracle import ppyolo_oracle as orc

PAD = 1
KINDS = ['integer +1', 'integer -2', 'half +0.5', 'half -1.5', 'on the lower bound', 'on the upper bound', '1 px below', '1 px above']


def out_hw(H, W, stride):
    return (H + 2 * PAD - 2) // stride, (W + 2 * PAD - 2) // stride


def tap_base(H, W, stride):
    """Un-offset sampling position of every (ho, wo, tap) in the padded frame -> (by, bx) [Ho, Wo, 9]."""
    Ho, Wo = out_hw(H, W, stride)
    kh = torch.arange(9) // 3
    kw = torch.arange(9) % 3
    by = (torch.arange(Ho) * stride + PAD).view(Ho, 1, 1) + (kh - 1).view(1, 1, 9)
    bx = (torch.arange(Wo) * stride + PAD).view(1, Wo, 1) + (kw - 1).view(1, 1, 9)
    return by.expand(Ho, Wo, 9).float(), bx.expand(Ho, Wo, 9).float()


def positions(case):
    """(py0, px0) [N, Ho, Wo, 9] before the clamp, and the bounds (ymax, xmax).  Exact in float32 for every case but 'random'."""
    N, H, W, C, K, stride = case['shape']
    by, bx = tap_base(H, W, stride)
    off = case['om'][:, :18].permute(0, 2, 3, 1).reshape(N, by.shape[0], by.shape[1], 9, 2)
    return by + off[..., 0], bx + off[..., 1], float(H + 2 * PAD - 1), float(W + 2 * PAD - 1)


def make(name, shape, seed, offsets='zero', mask='zero'):
    N, H, W, C, K, stride = shape
    Ho, Wo = out_hw(H, W, stride)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, 3, 3, C, generator=g) * (1.0 / (9 * C)) ** 0.5
    dy = torch.randn(N, K, Ho, Wo, generator=g)
    om = torch.zeros(N, Ho, Wo, 9, 3)                      # [..., tap, (off y, off x, mask logit)]
    by, bx = tap_base(H, W, stride)
    ymax, xmax = float(H + 2 * PAD - 1), float(W + 2 * PAD - 1)
    kinds = None
    if offsets == 'exact':
        kinds = torch.randint(0, len(KINDS), (N, Ho, Wo, 9, 2), generator=g)
        for d, (base, mx) in enumerate(((by, ymax), (bx, xmax))):
            table = torch.stack([torch.full_like(base, 1.0), torch.full_like(base, -2.0), torch.full_like(base, 0.5), torch.full_like(base, -1.5),
                                 -base, mx - base, -base - 1.0, mx - base + 1.0], -1)          # [Ho, Wo, 9, kinds]
            om[..., d] = torch.gather(table.expand(N, Ho, Wo, 9, len(KINDS)), -1, kinds[..., d:d + 1])[..., 0]
    elif offsets == 'collide':                             # every tap of every output pixel -> one fractional position at the centre
        om[..., 0] = (PAD + H // 2 + 0.3) - by
        om[..., 1] = (PAD + W // 2 + 0.6) - bx
    elif offsets == 'random':
        om[..., 0:2] = torch.randn(N, Ho, Wo, 9, 2, generator=g) * 1.5
    else:
        assert offsets == 'zero'
    if mask == 'random':
        om[..., 2] = torch.randn(N, Ho, Wo, 9, generator=g) * 2.0
    elif mask == 'one':
        om[..., 2] = 40.0                                  # sigmoid is exactly 1 in float32
    else:
        assert mask == 'zero'
    # the 27 channels of conv_offset's output: 18 offsets (y, x interleaved per tap), then 9 mask logits
    om27 = torch.cat([om[..., 0:2].reshape(N, Ho, Wo, 18), om[..., 2]], -1).permute(0, 3, 1, 2).contiguous()
    return dict(name=name, shape=shape, x=x, om=om27, w=w, dy=dy, stride=stride, kinds=kinds)


ZERO_SHAPES = [(3, 7, 6, 32, 32, 1), (2, 8, 10, 64, 72, 2), (8, 5, 5, 32, 32, 1)]
EXACT_SHAPES = [(2, 6, 7, 32, 40, 1), (3, 7, 8, 32, 32, 2)]
COLLIDE_SHAPE = (1, 9, 9, 32, 32, 1)
LAYOUT_SHAPES = [(2, 6, 6, 96, 32, 1), (2, 6, 6, 320, 40, 1)]       # C = 96: ragged last trip of the 64-lane loop; 320: a second trip of the 256-wide gather


def _shape_id(s):
    return 'x'.join(str(v) for v in s)


CASES = {}
for _i, _s in enumerate(ZERO_SHAPES):
    for _m in ('zero', 'random'):
        CASES['zero_%s_mask_%s' % (_shape_id(_s), _m)] = functools.partial(make, shape=_s, seed=200 + _i, offsets='zero', mask=_m)
for _i, _s in enumerate(EXACT_SHAPES):
    CASES['exact_%s' % _shape_id(_s)] = functools.partial(make, shape=_s, seed=210 + _i, offsets='exact', mask='random')
CASES['collide_%s' % _shape_id(COLLIDE_SHAPE)] = functools.partial(make, shape=COLLIDE_SHAPE, seed=220, offsets='collide', mask='random')
for _i, _s in enumerate(LAYOUT_SHAPES):
    CASES['layout_%s' % _shape_id(_s)] = functools.partial(make, shape=_s, seed=230 + _i, offsets='random', mask='random')


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name](name)


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=torch.float32):
    """-> dict(dx [N,C,H,W], dom [N,27,Ho,Wo], dw [K,3,3,C]) in `dtype` (shared: do not modify)."""
    c = get(name)
    N, H, W, C, K, stride = c['shape']
    x, om, w = (c[k].to(dtype).clone().requires_grad_(True) for k in ('x', 'om', 'w'))
    val = orc.dcnv2_sample(x, om[:, :18], torch.sigmoid(om[:, 18:]), stride, PAD)          # [N, Ho, Wo, 9, C]
    y = torch.einsum('nhwtc,ktc->nkhw', val, w.reshape(K, 9, C))
    y.backward(c['dy'].to(dtype))
    return dict(dx=x.grad, dom=om.grad, dw=w.grad)
