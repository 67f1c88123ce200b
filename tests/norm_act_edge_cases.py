"""Small adversarial calls of the GroupNorm / AffineChannel / Mish kernels (csrc/norm_act.hip, csrc/norm_act_train.hip) at the edges
of their launch geometry and of their values -- device-free TEST INFRASTRUCTURE (tests/test_norm_act_edge_cases.py checks the table's
own promises, its fairness and its power on the CPU, tests/test_gpu_norm_act_edges.py runs the kernels on it).

A Case names one family of calls: `op` is gn_fwd (ppy_group_norm_f32 plain and upsampled, ppy_group_norm_train_f32), gn_train_bwd
(ppy_group_norm_train_f32 then ppy_group_norm_bwd_f32, trained and frozen), affine_act_bwd (ppy_affine_act_f32 then
ppy_affine_bwd_f32, trained and frozen), mish (ppy_mish_f32) or mish_bwd (ppy_mish_bwd_f32).  `build()` returns the call's data as
CPU tensors -- every activation an ops.View over a CPU buffer: a channel slice of a wider buffer, outputs pre-filled with SENTINEL --
`why` says in one line what the call is for, `promise(kw)` asserts that the shape really reaches the branch `why` names, by the
launch arithmetic restated below, and that the data are what it claims.

Rules of the table: every case is a valid call (leading dimensions and channel offsets are multiples of 4 floats), no NaN / Inf
inputs, the smallest shapes that reach the branch.
"""
import collections
import zlib

import numpy as np
import torch

from ppyolo_hip import _lib, ops

SENTINEL = 7.25
EPS = 1e-5
ACTS = ('relu', 'leaky', 'mish', None)
OPS = ('gn_fwd', 'gn_train_bwd', 'affine_act_bwd', 'mish', 'mish_bwd')


# ---- the launch arithmetic of the entry points, restated ---------------------------------------------------------------------
# gn_forward (csrc/norm_act.hip) and ppy_group_norm_bwd_f32 with its gn_chunks (csrc/norm_act_train.hip) share one geometry;
# ppy_affine_bwd_f32 with its af_chunks (csrc/norm_act_train.hip) has its own.  The kernels that walk it: gn_partial_kernel,
# gn_bwd_partial_kernel, gn_bwd_combine_kernel, affine_bwd_kernel, affine_bwd_combine_kernel, reduce_pixels.
GN_MAX_CHUNKS = getattr(_lib, 'GN_MAX_CHUNKS', 128)          # PPY_GN_MAX_CHUNKS
AF_MAX_CHUNKS = 512                                          # AF_MAX_CHUNKS of csrc/norm_act_train.hip
MIN_CHUNK, THREADS, WAVE = 32, 256, 64


def ceil_div(a, b):
    return -(-a // b)


def _tx(Q):
    tx = 1
    while tx < Q and tx < 64:
        tx *= 2
    return tx


def gn_geometry(N, H, W, C, groups):
    """grid (nchunks, N, slabs) of the partial kernels, forward and backward, and what the combine walks."""
    P, Q, cpg = H * W, C // 4, C // groups
    rows_per = max(MIN_CHUNK, ceil_div(P, GN_MAX_CHUNKS))
    nchunks = ceil_div(P, rows_per)
    TX = _tx(Q)
    slabs = ceil_div(Q, TX) if (4 * TX) % cpg == 0 else 1
    passes = 1 if slabs > 1 else ceil_div(Q, TX)          # trips of a workgroup's loop over channel quads
    live_last = Q - (ceil_div(Q, TX) - 1) * TX            # live quad lanes of the last pass / of the last slab
    return dict(P=P, Q=Q, cpg=cpg, rows_per=rows_per, nchunks=nchunks, last_chunk=P - (nchunks - 1) * rows_per, TX=TX, TY=THREADS // TX,
                slabs=slabs, passes=passes, live_last=live_last, groups_per_slab=(4 * TX // cpg if slabs > 1 else groups),
                group_entries=nchunks, channel_entries=N * nchunks, lds_bytes=(THREADS * 8 + 2 * C) * 8)


def af_geometry(N, H, W, C):
    """grid (nchunks, slabs) of affine_bwd_kernel over the N * H * W pixels."""
    pixels, Q = N * H * W, C // 4
    rows_per = max(MIN_CHUNK, ceil_div(pixels, AF_MAX_CHUNKS))
    nchunks = ceil_div(pixels, rows_per)
    TX = _tx(Q)
    slabs = ceil_div(Q, TX)
    return dict(pixels=pixels, Q=Q, rows_per=rows_per, nchunks=nchunks, last_chunk=pixels - (nchunks - 1) * rows_per, TX=TX,
                TY=THREADS // TX, slabs=slabs, live_last=Q - (slabs - 1) * TX)


def raw_group_var(v):
    """E[x^2] - E[x]^2 of a group's values by plain double sums in element order, no shift: what the clamp var < 0 -> 0 is for."""
    d = v.double().reshape(-1).numpy()
    m = np.cumsum(d)[-1] / d.size
    return float(np.cumsum(d * d)[-1] / d.size - m * m)


# ---- the table ---------------------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, name, op, why, build, promise):
        self.name, self.op, self.why, self.build, self.promise = name, op, why, build, promise

    def __repr__(self):
        return 'Case(%s)' % self.name


CASES = collections.OrderedDict()


def _add(name, op, why, build, promise):
    assert name not in CASES and op in OPS, name
    CASES[name] = Case(name, op, why, build, promise)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def view(t, pad, off, fill=SENTINEL):
    """The NHWC tensor as the channel slice [off, off + C) of a buffer `pad` channels wider (CPU)."""
    N, H, W, C = t.shape
    buf = torch.full((N, H, W, C + pad), fill)
    buf[..., off:off + C] = t
    return ops.View(buf, off, C)


def dense(v):
    return v.t[..., v.coff:v.coff + v.C]


def outside_untouched(v, fill=SENTINEL):
    return bool((v.t[..., :v.coff] == fill).all()) and bool((v.t[..., v.coff + v.C:] == fill).all())


def _act_name(act, res):
    return '%s%s' % (act or 'none', '_res' if res else '')


def _gn_data(name, N, H, W, C, groups, act, with_res):
    """x (the last image scaled and shifted against the first), dy, residual, gamma, beta; x, dy, dx, y, dz and the residual each a
    channel slice of a wider buffer of its own pitch and offset."""
    gen = _gen(name)
    x = torch.randn(N, H, W, C, generator=gen)
    x[-1] = x[-1] * 2.5 - 0.75
    dy = torch.randn(N, H, W, C, generator=gen)
    res = torch.randn(N, H, W, C, generator=gen) if with_res else None
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    return dict(shape=(N, H, W, C), groups=groups, act=act, eps=EPS, value=None, x=x, dy=dy, res=res, gamma=gamma, beta=beta)


def gn_views(kw):
    """The ops.View objects of a GroupNorm case over fresh CPU buffers (inputs copied in, outputs at SENTINEL)."""
    N, H, W, C = kw['shape']
    z = torch.full((N, H, W, C), SENTINEL)
    return dict(x=view(kw['x'], 24, 8), dy=view(kw['dy'], 12, 4), res=None if kw['res'] is None else view(kw['res'], 8, 4),
                y=view(z, 20, 16), yu=view(torch.full((N, 2 * H, 2 * W, C), SENTINEL), 20, 16), dx=view(z, 24, 8), dz=view(z, 8, 4))


af_views = gn_views


def _geometry_promise(N, H, W, C, groups, want):
    def promise(kw):
        g = gn_geometry(N, H, W, C, groups)
        for k, v in want.items():
            assert g[k] == v, (k, g[k], v)
        assert kw['shape'] == (N, H, W, C) and g['nchunks'] <= GN_MAX_CHUNKS and g['lds_bytes'] <= 48 * 1024
        assert not torch.equal(kw['x'][0], kw['x'][-1]) or N == 1
    return promise


# (N, H, W, C, groups), the restated geometry the shape must give, what it reaches, two (activation, residual) variants
GN_GEOMETRY = [
    ((2, 47, 47, 32, 8), dict(nchunks=70, rows_per=32, last_chunk=1, group_entries=70, channel_entries=140),
     '70 chunks, the last of 1 pixel: the second trip of the combine lane loop for group items, 140 entries per channel item',
     [('relu', True), (None, False)]),
    ((1, 64, 64, 16, 4), dict(nchunks=128, rows_per=32, last_chunk=32), 'exactly PPY_GN_MAX_CHUNKS chunks of 32 pixels: the cap',
     [('leaky', False), ('mish', True)]),
    ((1, 65, 63, 16, 4), dict(nchunks=128, rows_per=32, last_chunk=31), '128 chunks, the last of 31 pixels',
     [('mish', False), ('relu', True)]),
    ((1, 70, 70, 8, 2), dict(nchunks=126, rows_per=39, last_chunk=25), 'rows_per 39 > 32 and 126 chunks, in the backward too',
     [(None, True), ('leaky', False)]),
    ((2, 5, 7, 320, 32), dict(cpg=10, slabs=1, passes=2, TX=64, live_last=16),
     '10 channels per group, no slabs: two passes of the 64 quad lanes, 16 live in the second', [('relu', False), ('leaky', True)]),
    ((2, 5, 7, 320, 5), dict(cpg=64, slabs=2, live_last=16, groups_per_slab=4),
     '64 per group: 2 slabs, the last with 16 of 64 quads and group 4 alone', [('leaky', True), ('mish', False)]),
    ((1, 3, 3, 768, 3), dict(cpg=256, slabs=3, groups_per_slab=1, live_last=64), '256 per group: 3 slabs of one group each',
     [('mish', True), (None, False)]),
    ((1, 3, 3, 2048, 8), dict(cpg=256, slabs=8, groups_per_slab=1, lds_bytes=48 * 1024), '8 slabs of one group each; LDS exactly 48 KB',
     [(None, True), ('relu', False)]),
    ((1, 2, 3, 2044, 7), dict(cpg=292, slabs=1, passes=8, live_last=63), '292 per group: 8 unslabbed passes, 63 live lanes in the last',
     [('mish', True), (None, False)]),
    ((2, 6, 6, 40, 4), dict(cpg=10, TX=16, slabs=1, passes=1, live_last=10), '10 per group, TX 16 with 10 live lanes',
     [('leaky', False), ('relu', True)]),
    ((2, 7, 5, 64, 1), dict(cpg=64, slabs=1, passes=1), 'one group over all channels', [('mish', False), ('leaky', True)]),
    ((2, 7, 5, 64, 64), dict(cpg=1, slabs=1, passes=1), 'one channel per group', [('relu', True), (None, False)]),
    ((2, 9, 9, 4, 2), dict(TX=1, TY=256, cpg=2, nchunks=3), 'TX 1: one lane along C, the 256-deep pixel tree',
     [('leaky', True), ('mish', False)]),
    ((2, 1, 33, 12, 3), dict(TX=4, live_last=3, nchunks=2, last_chunk=1), 'TX 4 with 3 live lanes; a second chunk of one pixel',
     [(None, True), ('relu', False)]),
]


def geometry_class(N, H, W, C, groups):
    g = gn_geometry(N, H, W, C, groups)
    return 'slabbed' if g['slabs'] > 1 else 'multi-pass' if g['passes'] > 1 else 'many-chunk' if g['nchunks'] > WAVE else 'other'


for _shape, _want, _why, _variants in GN_GEOMETRY:
    for _act, _res in _variants:
        for _op in ('gn_fwd', 'gn_train_bwd'):
            _dn = '%s_g%d_%s' % ('x'.join(str(v) for v in _shape[:4]), _shape[4], _act_name(_act, _res))          # both ops: the same data
            _add(_op + '_' + _dn, _op, _why, (lambda n=_dn, s=_shape, a=_act, r=_res: _gn_data(n, *s, act=a, with_res=r)),
                 _geometry_promise(*_shape, want=_want))


# ---- AffineChannel geometry --------------------------------------------------------------------------------------------------
def _af_data(name, N, H, W, C, act, with_res):
    gen = _gen(name)
    x = torch.randn(N, H, W, C, generator=gen) * 1.5 + 0.2
    x[-1] = x[-1] * 2.5 - 0.75
    dy = torch.randn(N, H, W, C, generator=gen)
    res = torch.randn(N, H, W, C, generator=gen) if with_res else None
    w, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    return dict(shape=(N, H, W, C), act=act, value=None, x=x, dy=dy, res=res, gamma=w, beta=b)


def _af_promise(N, H, W, C, want):
    def promise(kw):
        g = af_geometry(N, H, W, C)
        for k, v in want.items():
            assert g[k] == v, (k, g[k], v)
        assert kw['shape'] == (N, H, W, C) and g['nchunks'] <= AF_MAX_CHUNKS
    return promise


AF_GEOMETRY = [
    ((4, 64, 64, 8), dict(nchunks=512, rows_per=32, last_chunk=32), '512 chunks of 32 pixels: the cap', 'relu', True),
    ((5, 60, 60, 8), dict(nchunks=500, rows_per=36), 'rows_per 36 > 32, 500 chunks: eight trips of the combine lane loop', 'leaky', False),
    ((2, 5, 7, 320), dict(slabs=2, live_last=16, TX=64), 'two slabs in gridDim.y, 16 live lanes in the second', 'mish', True),
    ((3, 7, 5, 260), dict(slabs=2, live_last=1), 'one live lane in the second slab', None, False),
    ((1, 1, 1, 4), dict(nchunks=1, TX=1, slabs=1, last_chunk=1), 'the smallest shape', 'leaky', True),
]

for _shape, _want, _why, _act, _res in AF_GEOMETRY:
    _name = 'affine_%s_%s' % ('x'.join(str(v) for v in _shape), _act_name(_act, _res))
    _add(_name, 'affine_act_bwd', _why, (lambda n=_name, s=_shape, a=_act, r=_res: _af_data(n, *s, act=a, with_res=r)), _af_promise(*_shape, want=_want))


# ---- value cases -------------------------------------------------------------------------------------------------------------
VALUE_SHAPES = [(2, 13, 11, 64, 32), (2, 5, 7, 320, 5)]          # the base shape of the direct tests, and a slabbed one


def _group_slice(C, groups, g):
    cpg = C // groups
    return slice(g * cpg, (g + 1) * cpg)


def _large_mean(name, shape):
    kw = _gn_data(name, *shape, act='leaky', with_res=True)
    N, H, W, C = kw['shape']
    gsel = [1 % shape[4], (shape[4] - 1)][:N] + [0] * max(0, N - 2)          # one group per image
    twin = kw['x'].clone()
    for n in range(N):
        s = _group_slice(C, shape[4], gsel[n])
        twin[n, :, :, s] = 1e-2 * twin[n, :, :, s]
        kw['x'][n, :, :, s] = 1000.0 + twin[n, :, :, s]
        twin[n, :, :, s] = kw['x'][n, :, :, s] - 1000.0          # (float32: exact, see the promise)
    kw.update(value='large_mean', twin=twin, sel=gsel)
    return kw


def _large_mean_promise(shape):
    def promise(kw):
        N, H, W, C = kw['shape']
        assert geometry_class(*shape) == ('slabbed' if shape[3] > 256 else 'other')
        back = kw['twin'].double()
        for n in range(N):
            s = _group_slice(C, shape[4], kw['sel'][n])
            v = kw['x'][n, :, :, s].double()
            assert abs(float(v.mean()) - 1000.0) < 1e-2 and 1e-3 < float(v.std()) < 1e-1
            back[n, :, :, s] += 1000.0
            m32 = kw['x'][n, :, :, s].mean()          # float32 one-pass moments keep no digit of this variance
            one_pass = float((kw['x'][n, :, :, s] ** 2).mean() - m32 * m32)
            assert abs(one_pass - float(v.var(unbiased=False))) > 0.5 * float(v.var(unbiased=False))
        assert torch.equal(back, kw['x'].double()), 'x - 1000 must be exact in float32: the twin is the same data, shifted'
    return promise


def _constant_value(v_like):
    """A constant near 1000 whose raw (unshifted) double moments come out NEGATIVE on this group size, so that a missing clamp shows."""
    for i in range(64):
        v = torch.full_like(v_like, 997.1 + 0.37 * i)
        if raw_group_var(v) < -1e-10:
            return float(v.reshape(-1)[0])
    raise AssertionError('no constant with a negative raw variance')


def _constant_group(name, shape, act, with_res, zero_beta=False):
    kw = _gn_data(name, *shape, act=act, with_res=with_res)
    C, groups = shape[3], shape[4]
    g = groups - 1          # the last group: on the slabbed shape, the partial last slab
    s = _group_slice(C, groups, g)
    c = _constant_value(kw['x'][0, :, :, s])
    twin = kw['x'].clone()
    kw['x'][0, :, :, s] = c
    twin[0, :, :, s] = 0.0
    if zero_beta:
        kw['beta'][s] = 0.0
    kw.update(value='zero_preactivation' if zero_beta else 'constant_group', twin=twin, sel=(0, g), const=c)
    return kw


def _constant_promise(shape, zero_beta):
    def promise(kw):
        N, H, W, C = kw['shape']
        n, g = kw['sel']
        s = _group_slice(C, shape[4], g)
        v = kw['x'][n, :, :, s]
        assert v.numel() > 1 and bool((v == kw['const']).all()), 'one constant, m > 1'
        rv = raw_group_var(v)
        assert rv < -1e-10 and abs(rv) > 1e-6 * EPS, 'raw double moments go negative here: unclamped, rstd moves by %g' % (rv / EPS)
        assert torch.equal(kw['twin'][n, :, :, s], torch.zeros_like(v)) and not bool((kw['x'][1, :, :, s] == kw['const']).any())
        if zero_beta:
            assert kw['res'] is None and bool((kw['beta'][s] == 0).all()) and kw['act'] in ('relu', 'leaky')
    return promise


def _mish_tails(name, shape):
    kw = _gn_data(name, *shape, act='mish', with_res=False)
    kw['beta'][:8] = torch.tensor([25., -25., 90., -90., 20., -20., 21., -87.])
    kw['value'] = 'mish_tails'
    return kw


def _mish_tails_promise(shape):
    def promise(kw):
        N, H, W, C = kw['shape']
        x = kw['x'].permute(0, 3, 1, 2).double()
        g = x.reshape(N, shape[4], -1)
        xh = ((g - g.mean(2, keepdim=True)) / torch.sqrt(g.var(2, unbiased=False, keepdim=True) + EPS)).reshape(x.shape)
        z = xh * kw['gamma'].double().view(1, -1, 1, 1) + kw['beta'].double().view(1, -1, 1, 1)
        assert float((z[:, 0] > 20.0).double().mean()) > 0.9 and float(z[:, 2].min()) > 80.0, 'beyond the softplus threshold'
        assert float(z[:, 1].max()) < -15.0 and float(z[:, 3].max()) < -80.0, 'deep in the negative tail'
        assert float(z[:, 4].min()) < 20.0 < float(z[:, 4].max()), 'both sides of the threshold'
    return promise


def _independence(name):
    kw = _gn_data(name, 3, 47, 47, 32, 8, act='leaky', with_res=True)
    kw['x'][1] = kw['x'][0] * 1e3
    kw['value'] = 'image_independence'
    return kw


def _independence_promise(kw):
    g = gn_geometry(3, 47, 47, 32, 8)
    assert g['nchunks'] == 70 and g['channel_entries'] == 210
    assert torch.equal(kw['x'][1], kw['x'][0] * 1e3) and float(kw['x'][1].abs().max()) > 1e3


for _shape in VALUE_SHAPES:
    _tag = '%dc_g%d' % (_shape[3], _shape[4])
    _add('large_mean_' + _tag, 'gn_train_bwd', 'one group per image is 1000 + 1e-2 randn: the backward twin of test_group_norm_kernel_large_mean',
         (lambda n='large_mean_' + _tag, s=_shape: _large_mean(n, s)), _large_mean_promise(_shape))
    _add('constant_group_' + _tag, 'gn_train_bwd', 'one group of image 0 holds one constant: var == 0, rstd = 1 / sqrt(eps) = 316',
         (lambda n='constant_group_' + _tag, s=_shape: _constant_group(n, s, 'leaky', True)), _constant_promise(_shape, False))
    for _act in ('relu', 'leaky'):
        _add('zero_preactivation_%s_%s' % (_act, _tag), 'gn_train_bwd', 'a constant group with beta == 0: z is exactly 0 under ' + _act,
             (lambda n='zero_preactivation_%s_%s' % (_act, _tag), s=_shape, a=_act: _constant_group(n, s, a, False, zero_beta=True)),
             _constant_promise(_shape, True))
    _add('mish_tails_' + _tag, 'gn_train_bwd', 'beta of +-25 and +-90: z beyond the softplus threshold and deep in the negative tail',
         (lambda n='mish_tails_' + _tag, s=_shape: _mish_tails(n, s)), _mish_tails_promise(_shape))
_add('image_independence', 'gn_train_bwd', 'N = 3 on the 70-chunk shape, image 1 = 1e3 x image 0: every image equals its own run alone',
     lambda: _independence('image_independence'), _independence_promise)


# ---- sign-pattern cases ------------------------------------------------------------------------------------------------------
def _chosen(gen, N, H, W, C):
    """One element per channel: (n, h, w) for channel c."""
    return torch.stack([torch.randint(0, N, (C,), generator=gen), torch.randint(0, H, (C,), generator=gen),
                        torch.randint(0, W, (C,), generator=gen)], dim=1)


def chosen_of(t_nhwc, chosen):
    """The chosen element of every channel of an NHWC tensor -> [C]."""
    c = torch.arange(t_nhwc.shape[3])
    return t_nhwc[chosen[:, 0], chosen[:, 1], chosen[:, 2], c]


def _slope_gn(name, act, with_res):
    kw = _gn_data(name, 2, 13, 11, 64, 32, act=act, with_res=with_res)
    ch = _chosen(_gen(name + ' chosen'), 2, 13, 11, 64)
    kw['dy'] = torch.ones_like(kw['dy'])
    if with_res:
        kw['res'][ch[:, 0], ch[:, 1], ch[:, 2], torch.arange(64)] = 0.0
    kw.update(value='slope', chosen=ch)          # beta is set by the runner: -fl(xhat * gamma) of the chosen element AS THE DEVICE computes it
    return kw


def _slope_af(name, act):
    kw = _af_data(name, 2, 13, 11, 64, act=act, with_res=False)
    ch = _chosen(_gen(name + ' chosen'), 2, 13, 11, 64)
    kw['dy'] = torch.ones_like(kw['dy'])
    prod = chosen_of(kw['x'], ch).numpy().astype(np.float32) * kw['gamma'].numpy().astype(np.float32)          # float32 product, rounded once
    kw['beta'] = torch.from_numpy(-prod)
    kw.update(value='slope', chosen=ch)
    return kw


def _slope_promise(kw):
    ch = kw['chosen']
    assert ch.shape == (kw['shape'][3], 3) and bool((kw['dy'] == 1).all())
    if kw['res'] is not None:
        assert bool((chosen_of(kw['res'], ch) == 0).all())
    if 'groups' not in kw:
        x, w, b = (t.numpy() for t in (chosen_of(kw['x'], ch), kw['gamma'], kw['beta']))
        assert bool(((x * w).astype(np.float32) + b == 0).all()), 'without contraction z is exactly 0 at the chosen elements'
        resid = x.astype(np.float64) * w.astype(np.float64) + b.astype(np.float64)          # what a fused multiply-add leaves
        assert (resid != 0).mean() > 0.9 and (resid > 0).any() and (resid < 0).any()


for _act in ('relu', 'leaky'):
    for _res in (False, True):
        _n = 'slope_consistency_gn_' + _act_name(_act, _res)
        _add(_n, 'gn_train_bwd', 'z within one rounding of 0 at one element per channel: the backward must see the forward\'s signs',
             (lambda n=_n, a=_act, r=_res: _slope_gn(n, a, r)), _slope_promise)
    _n = 'slope_consistency_affine_' + _act
    _add(_n, 'affine_act_bwd', 'bias = -fl(x * weight) at one element per channel: the backward must see the forward\'s signs',
         (lambda n=_n, a=_act: _slope_af(n, a)), _slope_promise)


# ---- Mish ----------------------------------------------------------------------------------------------------------------------
MISH_PROBE = (-100., -90., -87., -25., -20., -1.1924, -1e-3, 0., 1e-3, 9.02, 19.99, 20., 20.01, 25., 88., 90., 100.)


def _mish_data(name, N, H, W, C, scale_shift=False):
    gen = _gen(name)
    x = torch.randn(N, H, W, C, generator=gen) * 8.0
    x[0, 0, 0, :len(MISH_PROBE)] = torch.tensor(MISH_PROBE)
    x[-1, -1, -1, -len(MISH_PROBE):] = torch.tensor(MISH_PROBE)          # the last quads of the last pixel
    kw = dict(shape=(N, H, W, C), x=x, dy=torch.randn(N, H, W, C, generator=gen), scale=None, shift=None, value=None)
    if not scale_shift:
        kw['dy'] = torch.ones(N, H, W, C)          # the 4-ulp rule is stated for the derivative itself
    else:
        kw['scale'], kw['shift'] = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    return kw


def _mish_promise(N, H, W, C, stride_loop):
    def promise(kw):
        quads = N * H * W * (C // 4)
        assert (quads > 2048 * THREADS) == stride_loop and quads % THREADS != 0          # stream_grid: 2048 workgroups at the most
        assert float(kw['x'].max()) > 20 and float(kw['x'].min()) < -87
    return promise


for _op in ('mish', 'mish_bwd'):
    _add(_op + '_2x9x9x68_tails', _op, 'the probe row (softplus threshold, expf range ends, the zero of the derivative) on a partial last workgroup',
         (lambda n=_op + '_tails': _mish_data(n, 2, 9, 9, 68)), _mish_promise(2, 9, 9, 68, False))
    _add(_op + '_1x181x181x68_stride', _op, 'more quads than 2048 workgroups hold: the second trip of the grid-stride loop, partly dead',
         (lambda n=_op + '_stride': _mish_data(n, 1, 181, 181, 68)), _mish_promise(1, 181, 181, 68, True))
_add('mish_bwd_2x9x9x68_scale_shift', 'mish_bwd', 'the pre-activation recomputed from a scale and a shift',
     (lambda: _mish_data('mish_bwd_scale', 2, 9, 9, 68, True)), _mish_promise(2, 9, 9, 68, False))


def mish_views(kw):
    z = torch.full(kw['shape'], SENTINEL)
    return dict(x=view(kw['x'], 12, 8), dy=view(kw['dy'], 4, 0), dx=view(z, 20, 16))
