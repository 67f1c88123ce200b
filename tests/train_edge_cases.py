"""Small adversarial calls of the training step's kernels (csrc/train.hip, csrc/conv_bwd.hip, the training entry points of
csrc/stem_pool.hip and the convolution library) for the launch-level float64 checkers of tests/launch_replay.py -- device-free TEST
INFRASTRUCTURE (tests/test_train_edge_cases.py checks the table's own promises, its fairness and its power on the CPU,
tests/test_gpu_train_edges.py runs the kernels on it).

A Case names one `ops.<op>` call: `build()` returns the call's keyword arguments with CPU tensors (ops.View objects over CPU
buffers where the op takes a View), `why` says in one line what the call is for, `promise(kw)` asserts that the data and the
restated launch arithmetic really are what `why` claims, `prep(ops, kw)` (contractions only) derives on the device what only the
library can make (operand planes, the prepared-weight table), `env` are environment switches the call runs under.

Rules of the table: every case is a valid call (leading dimensions and channel offsets are multiples of 4 floats wherever the entry
point loads 16 bytes); no NaN / Inf inputs; the smallest sizes that reach the code path, nothing larger than (8, 76, 76, 32, 64).
Output buffers are pre-filled with SENTINEL, slices sit at channel offset 4 of a buffer 12 or more channels wider.

The host-side launch arithmetic a case depends on is restated here in plain Python (slices_for / bn_slices, apply_ppb,
spp_bwd_fused, dropblock_tiled, wgrad_nine_tap) so that the host test can assert each promise instead of trusting a comment.
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

from ppyolo_hip import ops

SENTINEL = 7.5
DENORMAL = 1e-40                    # a float32 subnormal (2^-126 = 1.18e-38 is the smallest normal)
EPS, MOMENTUM = 1e-5, 0.1

# Ops with a checker in tests/launch_replay.py that this table leaves out, with the reason.
EXEMPT = {
    'yolov3_loss': 'edge suite of its own against the training oracle: tests/loss_cases.py, tests/test_gpu_loss_edges.py',
    'dcnv2': 'edge suite of its own against the DCNv2 oracle: tests/dcn_cases.py, tests/test_gpu_dcn_edges.py',
    'dcnv2_backward': 'edge suite of its own against the DCNv2 oracle: tests/dcn_cases.py, tests/test_gpu_dcn_edges.py',
    'stem_conv': 'judged against the oracle at its own edge shapes by the stem tests of tests/test_gpu_ops.py',
}


# ---- the launch arithmetic of the entry points, restated -------------------------------------------------------------------
BN_CH, BN_MAX_SLICES, SPP_CG, DB_TH, DB_CG = 64, 256, 4, 4, 32


def ceil_div(a, b):
    return -(-a // b)


def slices_for(P, C):
    """First estimate of the pixel-slice count of the statistics kernels (csrc/train.hip: slices_for)."""
    sl = min(ceil_div(1024, ceil_div(C, BN_CH)), max(P // 128, 1), BN_MAX_SLICES)
    return max(sl, 1)


def bn_slices(P, C):
    """-> (first estimate, pix_per_slice, re-derived slice count) of ppy_bn_train_stats_f32 / _bwd_f32 / ppy_channel_sum_f32."""
    s0 = slices_for(P, C)
    pps = ceil_div(P, s0)
    return s0, pps, ceil_div(P, pps)


def last_slice_pixels(P, C):
    _, pps, sl = bn_slices(P, C)
    return P - (sl - 1) * pps


def apply_ppb(P, C, hw):
    """Pixels per workgroup of bn_apply_kernel / bn_bwd_apply_kernel (ppy_bn_train_apply_f32); hw = pixels per image when a
    maximum is tracked, else P."""
    return min(max(ceil_div(P, 4096), ceil_div(4096, C)), hw)


def spp_bwd_fused(N, H, W):
    """ppy_spp_bwd_f32 runs as one launch when an image's maps fit the LDS."""
    return H * W * SPP_CG * (5 * 4 + 4 * 2) <= 150 * 1024 and N <= 65535


def dropblock_tiled(N, H, W, C):
    """ppy_dropblock_mask_f32 takes the tiled kernel when a row block with its halo fits 64 KiB."""
    tiles = N * ceil_div(H, DB_TH) * ceil_div(C, DB_CG)
    return (DB_TH + 2) * (W + 2) * DB_CG <= 64 * 1024 and tiles < 2 ** 31


def wgrad_nine_tap(C, R, S, stride, pad, f16x2, env=None):
    """The weight gradient runs with all nine taps in one workgroup (conv_wgrad9_kernel)."""
    off = (env or {}).get('PPY_WGRAD9', '1')[0] == '0'
    return f16x2 and not off and R == 3 and S == 3 and stride == 1 and pad == 1 and C % 32 == 0


def _first_P(pred, C=8, lo=129, hi=40000):
    for P in range(lo, hi):
        if pred(P, C):
            return P
    raise AssertionError('no such P')


P_LAST_SLICE_ONE = _first_P(lambda P, C: bn_slices(P, C)[2] > 1 and last_slice_pixels(P, C) == 1)      # 16513
P_FEWER_SLICES = _first_P(lambda P, C: bn_slices(P, C)[2] < bn_slices(P, C)[0])                         # 16641


def dropblock_mask_reference(N, H, W, C, keep, seed):
    """ppy_dropblock_mask_f32 bit for bit in numpy: the counter-based generator (one 64-bit hash per element id), gamma from the
    reference's formula (height only), mask = 1 - maxpool3x3(u < gamma).  -> the mask as NCHW float32 tensor."""
    ids = np.arange(N * H * W * C, dtype=np.uint64)
    with np.errstate(over='ignore'):
        key = (np.uint64(seed) ^ (ids * np.uint64(0xD1342543DE82EF95))) + np.uint64(0x9E3779B97F4A7C15)
        key = (key ^ (key >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        key = (key ^ (key >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        key = (key ^ (key >> np.uint64(31))) >> np.uint64(32)
    u = ((key >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).reshape(N, H, W, C)
    gamma = np.float32(H * H * (1 - keep)) / np.float32(9 * (H - 2) ** 2)
    seeds = torch.from_numpy((u < gamma).astype(np.float32)).permute(0, 3, 1, 2)
    return 1.0 - F.max_pool2d(seeds, 3, 1, 1)


# ---- the table ---------------------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, name, op, why, build, promise, prep=None, env=None):
        self.name, self.op, self.why, self.build, self.promise, self.prep, self.env = name, op, why, build, promise, prep, env or {}

    def __repr__(self):
        return 'Case(%s)' % self.name


CASES = collections.OrderedDict()


def _add(name, op, why, build, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, op, why, build, **kw)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def wide(dense, extra=12, off=4):
    """The dense NHWC tensor as the channel slice [off, off + C) of a buffer `extra` channels wider, SENTINEL elsewhere."""
    C = dense.shape[-1]
    buf = torch.full(tuple(dense.shape[:-1]) + (C + extra,), SENTINEL)
    buf[..., off:off + C] = dense
    return ops.View(buf, off, C)


def view(dense, sliced, extra=12):
    return wide(dense, extra) if sliced else ops.View(dense.contiguous())


def out_like(shape, sliced, extra=12):
    return view(torch.full(shape, SENTINEL), sliced, extra)


def dense(v):
    return v.t[..., v.coff:v.coff + v.C]


# -- BatchNorm ---------------------------------------------------------------------------------------------------------------
BN_SPECIAL = ('large mean', 'const 0.25', 'const 1000', 'scale 1e-6', 'scale 1e4', 'outlier')


def bn_values(N, H, W, C, g):
    """NHWC activations whose first channels carry the value edges of BN_SPECIAL (as many as C has room for): mean 1e3 with spread
    1e-2; the constants 0.25 and 1000 (every partial sum exact, variance exactly 0, invstd = 1 / sqrt(eps)); scales 1e-6 and 1e4;
    one 1e4 outlier in an N(0, 1) channel.  The other channels: N(1.5, 3)."""
    x = torch.randn(N, H, W, C, generator=g) * 3 + 1.5
    sp = [1e3 + 1e-2 * torch.randn(N, H, W, generator=g), torch.full((N, H, W), 0.25), torch.full((N, H, W), 1000.0),
          1e-6 * torch.randn(N, H, W, generator=g), 1e4 * torch.randn(N, H, W, generator=g), torch.randn(N, H, W, generator=g)]
    sp[5].view(-1)[(N * H * W) // 2] = 1e4
    for i, t in enumerate(sp[:min(C, len(sp))]):
        x[..., i] = t
    return x


def _stats_of(x):
    xx = x.double().reshape(-1, x.shape[-1])
    m = xx.mean(0)
    v = ((xx - m) ** 2).mean(0)
    return m.float(), (1.0 / (v + EPS).sqrt()).float()


def _bn_stats(shape, sliced=False, running=True, seed=0, scalar_ld=False):
    def build():
        N, H, W, C = shape
        g = _gen(1000 + seed)
        x = bn_values(N, H, W, C, g)
        if scalar_ld:                    # ld = C + 3: not a multiple of 4 -> the scalar loads of the statistics kernel
            buf = torch.full((N, H, W, C + 3), SENTINEL)
            buf[..., 2:2 + C] = x
            xv = ops.View(buf, 2, C)
        else:
            xv = view(x, sliced)
        kw = collections.OrderedDict(x=xv, eps=EPS, momentum=MOMENTUM, mean=torch.full((C,), SENTINEL), invstd=torch.full((C,), SENTINEL),
                                     running_mean=torch.randn(C, generator=g) if running else None,
                                     running_var=torch.rand(C, generator=g) + 0.5 if running else None)
        return kw
    return build


def _promise_large_mean(kw):
    """The one-pass variance E[x^2] - E[x]^2 in float32 of the large-mean channel is off by more than the variance itself, and the
    constant channels have variance exactly 0."""
    x = dense(kw['x']).reshape(-1, kw['x'].C)
    P = x.shape[0]
    if P >= 17:
        c0 = x[:, 0]
        var = float(c0.double().var(unbiased=False))
        one_pass = float((c0 * c0).mean() - c0.mean() * c0.mean())
        assert abs(one_pass - var) > var, (one_pass, var)
    assert float(x[:, 1].double().var(unbiased=False)) == 0.0 and float(x[:, 2].double().var(unbiased=False)) == 0.0


def _all(*promises):
    def promise(kw):
        for p in promises:
            r = p(kw)
            assert r is None or r, p
    return promise


P_THRESHOLDS = (1, 2, 17, 127, 128, 129, 255, 256, 257)          # P / 128 = 0 | 1 | 2: one slice up to 255, two full slices at 256


def _promise_slices(count=None, sliced=None):
    """The slice count of the reduction by the restated arithmetic: max(1, P / 128) when not given; x is / is not a slice at offset 4."""
    def promise(kw):
        x = kw['x'] if 'x' in kw else kw['dy']
        P = x.N * x.H * x.W
        s0, pps, sl = bn_slices(P, x.C)
        assert sl == (max(1, P // 128) if count is None else count) and (sl - 1) * pps < P <= sl * pps, (P, s0, pps, sl)
        if sliced is not None:
            assert (x.coff == 4 and x.ld >= x.C + 12) == sliced
    return promise


def _promise_pitches(*keys):
    """The named operands are slices at offset 4 of buffers of pairwise different pitch, SENTINEL outside the slice."""
    def promise(kw):
        vs = [kw[k] for k in keys if kw[k] is not None]
        assert len({v.ld for v in vs}) == len(vs) and all(v.coff == 4 and v.ld >= v.C + 12 and v.ld % 4 == 0 for v in vs)
        for v in vs:
            assert bool((v.t[..., :4] == SENTINEL).all()) and bool((v.t[..., v.coff + v.C:] == SENTINEL).all())
    return promise


for _i, _P in enumerate(P_THRESHOLDS):
    _add('bn_stats_P%d' % _P, 'bn_train_stats', 'P = %d: the P / 128 slice thresholds (%d slices of %d pixels); value edges per channel'
         % ((_P,) + bn_slices(_P, 8)[2:0:-1]), _bn_stats((1, 1, _P, 8), sliced=bool(_i & 1), running=not (_i & 1), seed=_i),
         promise=_all(_promise_large_mean, _promise_slices(sliced=bool(_i & 1)), lambda kw, r=not (_i & 1): (kw['running_mean'] is not None) == r))


def _promise_last_one(kw):
    x = kw['x']
    assert last_slice_pixels(x.N * x.H * x.W, x.C) == 1 and bn_slices(x.N * x.H * x.W, x.C)[2] > 1


def _promise_fewer(kw):
    x = kw['x']
    s0, _, s1 = bn_slices(x.N * x.H * x.W, x.C)
    assert s1 < s0


_add('bn_stats_last_slice_one_pixel', 'bn_train_stats', 'P = %d: the last of %d slices holds a single pixel' % (P_LAST_SLICE_ONE, bn_slices(P_LAST_SLICE_ONE, 8)[2]),
     _bn_stats((1, 1, P_LAST_SLICE_ONE, 8), seed=20), promise=_promise_last_one)
_add('bn_stats_fewer_slices', 'bn_train_stats', 'P = %d: the re-derived slice count %d is below the first estimate %d'
     % (P_FEWER_SLICES, bn_slices(P_FEWER_SLICES, 8)[2], bn_slices(P_FEWER_SLICES, 8)[0]), _bn_stats((1, 1, P_FEWER_SLICES, 8), seed=21, running=False),
     promise=_promise_fewer)
for _i, _C in enumerate((4, 60, 64, 68, 1028)):
    _add('bn_stats_C%d' % _C, 'bn_train_stats', 'C = %d (partial 64- / 16-channel blocks), x a slice at offset 4 of a wider buffer, 2 slices' % _C,
         _bn_stats((2, 10, 15, _C), sliced=True, running=bool(_i & 1), seed=30 + _i),
         promise=_all(_promise_slices(2, sliced=True), lambda kw, C=_C: kw['x'].C == C and (C % 64 != 0 or C == 64)))
_add('bn_stats_C258_scalar', 'bn_train_stats', 'C = 258 in a buffer with ld = 261: the scalar loads of the statistics kernel',
     _bn_stats((2, 3, 5, 258), scalar_ld=True, seed=40), promise=lambda kw: kw['x'].ld == 261 and kw['x'].ld % 4 != 0 and kw['x'].C == 258)


def _merge_case(slices, C, seed):
    def build():
        g = _gen(1100 + seed)
        n = torch.randint(1, 200, (slices, 1), generator=g).float().expand(slices, C)
        m = torch.randn(slices, C, generator=g) * 2 + 1
        m2 = torch.rand(slices, C, generator=g) * n * 3
        m[:, 0], m2[:, 0] = 1e3 + 1e-2 * torch.randn(slices, generator=g), 1e-4 * n[:, 0]          # large mean, small spread
        m[:, 1], m2[:, 1] = 0.25, 0.0                                                               # constant channel
        part = torch.stack([n, m, m2], dim=2).reshape(-1)
        groups = ceil_div(slices, 64) if slices > 256 else 0
        buf = torch.full(((slices + groups) * C * 3,), SENTINEL)
        buf[:part.numel()] = part
        return collections.OrderedDict(partials=buf, slices=slices, eps=EPS, momentum=MOMENTUM, mean=torch.full((C,), SENTINEL),
                                       invstd=torch.full((C,), SENTINEL), running_mean=torch.randn(C, generator=g),
                                       running_var=torch.rand(C, generator=g) + 0.5)
    return build


for _sl, _C in ((1, 4), (17, 20), (256, 16), (257, 68)):
    _add('bn_merge_s%d_C%d' % (_sl, _C), 'bn_train_stats_merge', '%d slices (one- / two-level merge at 256 | 257), C = %d' % (_sl, _C),
         _merge_case(_sl, _C, _sl),
         promise=lambda kw, sl=_sl, C=_C: kw['slices'] == sl and kw['mean'].numel() == C
         and kw['partials'].numel() == (sl + (ceil_div(sl, 64) if sl > 256 else 0)) * C * 3 and bool((kw['partials'][:sl * C * 3] != SENTINEL).all()))


def _peaks(x, signed=False):
    """Image n: 10 (n + 1) on its LAST pixel, 10 n + 8 on its FIRST pixel (another channel) -- the largest value of every image sits
    on its last pixel, and a larger one follows on the next image's first pixel.  signed: the sign alternates from image to image
    (the per-channel sums of a gradient stay small, so the BatchNorm backward keeps the peaks where they are)."""
    N, H, W, C = x.shape
    flat = x.view(N, H * W, C)
    for n in range(N):
        s = -1.0 if signed and n & 1 else 1.0
        if n:
            flat[n, 0, 1] = s * (10.0 * n + 8.0)
        flat[n, H * W - 1, C - 2] = s * 10.0 * (n + 1)
    return x


def preloaded_amax(N):
    """A tracked-maximum block with 45 in one slot of every image: above the maxima of images 0..3 of _peaks, below the others'."""
    a = torch.zeros(N * ops.AMAX_FLOATS_PER_IMAGE)
    a.view(N, -1)[:, 5 * 16] = 45.0
    return a


def _identity_params(C, neg=False):
    gamma = torch.ones(C)
    if neg:
        gamma[1::2] = -1.0
    return torch.zeros(C), torch.ones(C), gamma, torch.zeros(C)


def _bn_apply_amax(N, H, W, C, seed):
    def build():
        g = _gen(1200 + seed)
        x = _peaks(torch.randn(N, H, W, C, generator=g) * 0.1)
        mean, invstd, gamma, beta = _identity_params(C)
        return collections.OrderedDict(x=wide(x, 12), mean=mean, invstd=invstd, gamma=gamma, beta=beta, y=out_like((N, H, W, C), True, 20),
                                       act='leaky', residual=None, amax_out=preloaded_amax(N))
    return build


def _promise_ppb_clamps(kw):
    x = kw['x']
    hw = x.H * x.W
    assert apply_ppb(x.N * hw, x.C, hw) == hw
    _promise_peaks(kw)


def _promise_peaks(kw):
    x = kw['x']
    a = dense(x).abs().reshape(x.N, x.H * x.W, -1).amax(dim=2)
    for n in range(x.N):
        assert int(a[n].argmax()) == x.H * x.W - 1 and float(a[n].max()) == 10.0 * (n + 1)
    pre = kw.get('amax_out', kw.get('amax_dx')).view(x.N, -1).amax(dim=1)
    assert bool((pre > a.amax(dim=1)).any()) and bool((pre < a.amax(dim=1)).any())


def _promise_straddle(kw):
    x = kw['x']
    hw = x.H * x.W
    ppb = apply_ppb(x.N * hw, x.C, hw)
    assert ppb == 64 and (1 * ppb) // hw == 0 and (2 * ppb - 1) // hw == 1 and hw % ppb != 0      # workgroup [64, 128): images 0 and 1
    _promise_peaks(kw)


for _hw in (1, 2, 3, 5):
    _add('bn_apply_amax_hw%d' % _hw, 'bn_train_apply', 'N = 9, H W = %d: ppb clamps to the image; maxima on last / next-first pixels, pre-loaded slots' % _hw,
         _bn_apply_amax(9, 1, _hw, 8, _hw), promise=_promise_ppb_clamps)
_add('bn_apply_amax_straddle', 'bn_train_apply', 'N = 9, 10 x 10, C = 64: ppb = 64, workgroups straddle two images mid-wave',
     _bn_apply_amax(9, 10, 10, 64, 9), promise=_promise_straddle)


def _bn_apply(shape, act, res, seed, amax=False):
    def build():
        N, H, W, C = shape
        g = _gen(1300 + seed)
        x = bn_values(N, H, W, C, g)
        mean, invstd = _stats_of(x)
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        gamma[::3] *= -1
        r = wide(torch.randn(N, H, W, C, generator=g), 24) if res else None
        return collections.OrderedDict(x=wide(x, 12), mean=mean, invstd=invstd, gamma=gamma, beta=beta, y=out_like(shape, True, 16), act=act,
                                       residual=r, amax_out=ops.amax_slots(N=N) if amax else None)
    return build


for _i, _C in enumerate((4, 60, 64, 68, 1028)):
    _add('bn_apply_C%d' % _C, 'bn_train_apply', 'C = %d (c4 = %d threads of work per pixel), a different pitch per operand, value edges' % (_C, _C // 4),
         _bn_apply((2, 3, 5, _C), (None, 'relu', 'leaky')[_i % 3], bool(_i & 1), _i, amax=bool(_i & 2)),
         promise=_all(_promise_pitches('x', 'y', 'residual'), lambda kw, C=_C: kw['x'].C == C and (C // 4 > 256) == (C == 1028),
                      lambda kw, r=bool(_i & 1), a=bool(_i & 2): (kw['residual'] is not None) == r and (kw['amax_out'] is not None) == a))
for _i, _P in enumerate(P_THRESHOLDS):
    _add('bn_apply_P%d' % _P, 'bn_train_apply', 'P = %d, C = 8: %d workgroup(s) of at most %d pixels' % (_P, ceil_div(_P, apply_ppb(_P, 8, _P)), apply_ppb(_P, 8, _P)),
         _bn_apply((1, 1, _P, 8), ('leaky', None, 'relu')[_i % 3], bool(_i & 1), 50 + _i),
         promise=lambda kw, P=_P: kw['x'].W == P and apply_ppb(P, 8, P) == min(512, P) and kw['amax_out'] is None)


def zero_edge_values(N, H, W, C, positive_denormals_only):
    """+0, -0 and denormals of both signs (positive only where the op would multiply a negative one by 0.1: that product is not
    exact) at chosen pixels of an N(0, 1) tensor."""
    x = torch.randn(N, H, W, C, generator=_gen(N * 1000 + H * 100 + W * 10 + C))
    f = x.view(-1, C)
    f[0, 0], f[0, 1], f[0, 2], f[0, 3] = 0.0, -0.0, DENORMAL, DENORMAL if positive_denormals_only else -DENORMAL
    f[-1, 0], f[-1, 1], f[-1, 2], f[-1, 3] = -0.0, 0.0, 3 * DENORMAL if positive_denormals_only else -3 * DENORMAL, DENORMAL
    return x


def _promise_zero_edges(key):
    def promise(kw):
        v = dense(kw[key]).reshape(-1, kw[key].C)
        assert float(v[0, 0]) == 0.0 and float(v[0, 1]) == 0.0 and {math.copysign(1.0, float(v[0, 0])), math.copysign(1.0, float(v[0, 1]))} == {1.0, -1.0}
        assert 0.0 < abs(float(v[0, 2])) < 2.0 ** -126
    return promise


def _bn_apply_zero(act, res):
    def build():
        N, H, W, C = 1, 2, 4, 8
        x = zero_edge_values(N, H, W, C, act == 'leaky')
        mean, invstd, gamma, beta = _identity_params(C, neg=True)
        if act == 'leaky':                   # the denormals times gamma stay positive (0.1 times a negative denormal is not exact)
            x.view(-1, C)[0, 2:4] *= gamma[2:4]
            x.view(-1, C)[-1, 2:4] *= gamma[2:4]
        r = None
        if res:
            rr = torch.randn(N, H, W, C, generator=_gen(7))
            rr.view(-1, C)[0] = 0.0
            rr.view(-1, C)[-1] = 0.0
            r = wide(rr, 16)
        return collections.OrderedDict(x=wide(x, 12), mean=mean, invstd=invstd, gamma=gamma, beta=beta, y=out_like((N, H, W, C), True, 24),
                                       act=act, residual=r, amax_out=None)
    return build


for _act in (None, 'relu', 'leaky'):
    for _res in (False, True):
        _add('bn_apply_zero_%s_%s' % (_act, 'res' if _res else 'nores'), 'bn_train_apply',
             'mean 0, invstd 1, gamma +-1, beta 0: y is exactly +-0 and a denormal at chosen pixels; act %s, residual %s' % (_act, _res),
             _bn_apply_zero(_act, _res), promise=_promise_zero_edges('x'))


def act_f32(z, act):
    if act == 'relu':
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == 'leaky':
        return torch.where(z > 0, z, z * 0.1)
    return z


def _bn_bwd(shape, act, seed, amax=None, y_zero=False, sliced=True):
    def build():
        N, H, W, C = shape
        g = _gen(1400 + seed)
        x = bn_values(N, H, W, C, g)
        mean, invstd = _stats_of(x)
        gamma = torch.rand(C, generator=g) + 0.5
        gamma[::3] *= -1
        beta = torch.randn(C, generator=g)
        y = act_f32((x - mean) * (invstd * gamma) + beta, act)
        if y_zero:
            y = zero_edge_values(N, H, W, C, False)
        dy = torch.randn(N, H, W, C, generator=g)
        am = None
        if amax == 'peaks':                 # x small around mean 0, invstd = gamma = 1, slope 1 everywhere: dx = dy up to O(sum(dy) / P)
            x = 0.01 * torch.randn(N, H, W, C, generator=g)
            y = x.abs() + 1.0
            dy = _peaks(dy * 0.01, signed=True)
            am = preloaded_amax(N)
            mean, gamma, invstd = torch.zeros(C), torch.ones(C), torch.ones(C)
        elif amax:
            am = ops.amax_slots(N=N)
        return collections.OrderedDict(x=view(x, sliced, 12), y=view(y, sliced, 16), dy=view(dy, sliced, 20), mean=mean, invstd=invstd, gamma=gamma,
                                       dx=out_like(shape, sliced, 24), dgamma=torch.full((C,), SENTINEL), dbeta=torch.full((C,), SENTINEL), act=act,
                                       ws=None, amax_dx=am)
    return build


def bn_bwd_dx64(kw):
    """dx of bn_train_bwd in float64 (the formula of the checker)."""
    x, y, dy = dense(kw['x']).double(), dense(kw['y']).double(), dense(kw['dy']).double()
    C = x.shape[-1]
    P = x.numel() // C
    neg = {None: 1.0, 'relu': 0.0, 'leaky': 0.1}[kw['act']]
    dz = (dy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, neg))).reshape(P, C)
    xh = (x.reshape(P, C) - kw['mean'].double()) * kw['invstd'].double()
    dx = kw['gamma'].double() * kw['invstd'].double() * (dz - (dz.sum(0) + xh * (dz * xh).sum(0)) / P)
    return dx.view(x.shape)


def _promise_bwd_peaks(kw):
    x = kw['x']
    hw = x.H * x.W
    a = bn_bwd_dx64(kw).abs().reshape(x.N, hw, -1).amax(dim=2)
    for n in range(x.N):
        assert int(a[n].argmax()) == hw - 1, (n, a[n])
    for n in range(x.N - 1):
        assert float(a[n + 1, 0]) > float(a[n].max()) or hw == 1
    pre = kw['amax_dx'].view(x.N, -1).amax(dim=1)
    assert bool((pre > a.amax(dim=1)).any()) and bool((pre < a.amax(dim=1)).any())
    ppb = apply_ppb(x.N * hw, x.C, hw)
    assert ppb == (hw if hw < 64 else 64)


for _i, _C in enumerate((4, 60, 64, 68, 1028)):
    _add('bn_bwd_C%d' % _C, 'bn_train_bwd', 'C = %d, x / y / dy / dx slices with a different pitch each, value edges, 2 slices' % _C,
         _bn_bwd((2, 10, 15, _C), (None, 'relu', 'leaky')[_i % 3], _i, amax=bool(_i & 1)),
         promise=_all(_promise_slices(2), _promise_pitches('x', 'y', 'dy', 'dx'), lambda kw, C=_C: kw['x'].C == C))
for _i, _P in enumerate(P_THRESHOLDS):
    _add('bn_bwd_P%d' % _P, 'bn_train_bwd', 'P = %d: the P / 128 slice thresholds of the backward sums (%d slices of %d pixels)' % ((_P,) + bn_slices(_P, 8)[2:0:-1]),
         _bn_bwd((1, 1, _P, 8), ('leaky', 'relu', None)[_i % 3], 10 + _i, sliced=bool(_i & 1)), promise=_promise_slices(sliced=bool(_i & 1)))
_add('bn_bwd_fewer_slices', 'bn_train_bwd', 'P = %d: the re-derived slice count %d of the backward sums is below the first estimate %d'
     % (P_FEWER_SLICES, bn_slices(P_FEWER_SLICES, 8)[2], bn_slices(P_FEWER_SLICES, 8)[0]), _bn_bwd((1, 1, P_FEWER_SLICES, 8), 'relu', 21, sliced=False),
     promise=_promise_fewer)
_add('bn_bwd_last_slice_one_pixel', 'bn_train_bwd', 'P = %d: the last slice of the backward sums holds a single pixel' % P_LAST_SLICE_ONE,
     _bn_bwd((1, 1, P_LAST_SLICE_ONE, 8), 'leaky', 20, sliced=False), promise=_promise_last_one)
for _act in (None, 'relu', 'leaky'):
    _add('bn_bwd_zero_%s' % _act, 'bn_train_bwd', 'y given as +-0 and denormals: the slope at 0 is the negative side\'s; act %s' % _act,
         _bn_bwd((1, 2, 4, 8), _act, 30, y_zero=True), promise=_promise_zero_edges('y'))
for _hw in (1, 2, 3, 5):
    _add('bn_bwd_amax_hw%d' % _hw, 'bn_train_bwd', 'N = 9, H W = %d: ppb clamps to the image; max|dx| per image with pre-loaded slots' % _hw,
         _bn_bwd((9, 1, _hw, 8), None, 40 + _hw, amax='peaks'), promise=_promise_bwd_peaks)
_add('bn_bwd_amax_straddle', 'bn_train_bwd', 'N = 9, 10 x 10, C = 64: ppb = 64, workgroups straddle two images mid-wave',
     _bn_bwd((9, 10, 10, 64), 'leaky', 49, amax='peaks'), promise=_promise_bwd_peaks)


# -- element-wise ops, copies and small reductions ---------------------------------------------------------------------------------
def _act_bwd(act):
    def build():
        N, H, W, C = 1, 2, 3, 4
        y = zero_edge_values(N, H, W, C, False)
        dy = torch.randn(N, H, W, C, generator=_gen(50))
        return collections.OrderedDict(dy=wide(dy, 12), y=wide(y, 16), dx=out_like((N, H, W, C), True, 20), act=act)
    return build


for _act in (None, 'relu', 'leaky'):
    _add('act_bwd_%s' % _act, 'act_bwd', 'C = 4 slices; y = +-0 and denormals take the negative side\'s slope; act %s' % _act, _act_bwd(_act),
         promise=_promise_zero_edges('y'))


def _add_inplace():
    N, H, W, C = 2, 1, 3, 4
    return collections.OrderedDict(dst=wide(zero_edge_values(N, H, W, C, False), 12), src=wide(zero_edge_values(N, H, W + 0, C, True).flip(0), 20))


_add('add_inplace_C4', 'add_inplace', 'C = 4, dst and src slices of different pitch, +-0 and denormal operands', _add_inplace,
     promise=_promise_zero_edges('dst'))


def _dropblock_apply(exact_scale):
    def build():
        N, H, W, C = 2, 3, 3, 4
        g = _gen(60)
        x = zero_edge_values(N, H, W, C, False) if exact_scale else torch.randn(N, H, W, C, generator=g)
        mask = (torch.rand(N, H, W, C, generator=g) < 0.8).float()
        scale = torch.tensor([2.0 if exact_scale else mask.numel() / float(mask.sum())])
        return collections.OrderedDict(x=wide(x, 12), mask=mask, scale=scale, y=out_like((N, H, W, C), True, 16))
    return build


_add('dropblock_apply_zeros', 'dropblock_apply', 'C = 4 slices, +-0 and denormals times a power-of-two scale (exact)', _dropblock_apply(True),
     promise=_promise_zero_edges('x'))
_add('dropblock_apply_scale', 'dropblock_apply', 'C = 4 slices, scale = numel / sum(mask)', _dropblock_apply(False),
     promise=_all(_promise_pitches('x', 'y'), lambda kw: kw['x'].C == 4 and 0 < float(kw['mask'].sum()) < kw['mask'].numel()
                  and float(kw['scale']) == float(torch.tensor(kw['mask'].numel() / float(kw['mask'].sum()))) and bool(((kw['mask'] == 0) | (kw['mask'] == 1)).all())))


def _upsample(shape, sliced):
    def build():
        N, H, W, C = shape
        x = torch.randn(N, H, W, C, generator=_gen(70 + W))
        return collections.OrderedDict(x=view(x, sliced, 12), y=out_like((N, 2 * H, 2 * W, C), sliced, 16))
    return build


def _upsample_bwd(shape, sliced, accumulate):
    def build():
        N, H, W, C = shape
        g = _gen(80 + W)
        dy = torch.randn(N, 2 * H, 2 * W, C, generator=g)
        dx = torch.randn(N, H, W, C, generator=g) + 3.0           # non-zero: accumulate adds onto it, plain overwrites it
        return collections.OrderedDict(dy=view(dy, sliced, 16), dx=view(dx, sliced, 12), accumulate=accumulate)
    return build


for _shape, _sl in (((1, 1, 1, 4), False), ((2, 3, 5, 8), True)):
    _tag = '%dx%d' % _shape[1:3]
    _add('upsample2x_%s' % _tag, 'upsample2x', '%s map (odd W / a single pixel), %s' % (_tag, 'slices' if _sl else 'dense'), _upsample(_shape, _sl),
         promise=lambda kw, sl=_sl: (kw['x'].H * kw['x'].W == 1 or kw['x'].W % 2 == 1) and (kw['y'].H, kw['y'].W) == (2 * kw['x'].H, 2 * kw['x'].W)
         and (kw['x'].coff == 4) == sl and (kw['y'].coff == 4) == sl and bool((kw['y'].t == SENTINEL).all()))
    for _acc in (False, True):
        _add('upsample2x_bwd_%s_%s' % (_tag, 'acc' if _acc else 'set'), 'upsample2x_bwd',
             '%s map onto a non-zero dx, accumulate %s' % (_tag, _acc), _upsample_bwd(_shape, _sl, _acc),
             promise=lambda kw, acc=_acc: bool((dense(kw['dx']) != 0).all()) and kw['accumulate'] == acc and kw['dy'].H == 2 * kw['dx'].H)


def _avgpool(H, W):
    def build():
        x = torch.randn(2, H, W, 4, generator=_gen(90 + H * 8 + W))
        return collections.OrderedDict(x=wide(x, 12), y=out_like((2, H // 2, W // 2, 4), True, 16))
    return build


def _avgpool_bwd(H, W):
    def build():
        dy = torch.randn(2, H // 2, W // 2, 4, generator=_gen(100 + H * 8 + W))
        return collections.OrderedDict(dy=wide(dy, 16), dx=out_like((2, H, W, 4), True, 12))
    return build


for _H in (2, 3, 5):
    for _W in (2, 3, 5):
        _add('avgpool2x2_%dx%d' % (_H, _W), 'avgpool2x2', '%d x %d: floor mode, the odd last row / column is not read' % (_H, _W), _avgpool(_H, _W),
             promise=lambda kw, H=_H, W=_W: (kw['x'].H, kw['x'].W, kw['y'].H, kw['y'].W) == (H, W, H // 2, W // 2) and bool((kw['y'].t == SENTINEL).all()))
        _add('avgpool2x2_bwd_%dx%d' % (_H, _W), 'avgpool2x2_bwd', '%d x %d: the odd last row / column of dx is exactly 0' % (_H, _W), _avgpool_bwd(_H, _W),
             promise=lambda kw, H=_H, W=_W: (kw['dx'].H, kw['dx'].W, kw['dy'].H, kw['dy'].W) == (H, W, H // 2, W // 2)
             and bool((kw['dx'].t != 0).all()))          # (dx starts non-zero: an odd row that comes out 0 was written)


def _zero_insert(stride, beyond):
    def build():
        N, Ho, Wo, K = 2, 3, 4, 6
        H1, W1 = (Ho - 1) * stride + 1 + beyond, (Wo - 1) * stride + 1 + beyond
        dy = torch.randn(N, Ho, Wo, K, generator=_gen(110 + stride))
        return collections.OrderedDict(dy=wide(dy, 10, 3), up=out_like((N, H1, W1, K), True, 26), stride=stride)
    return build


for _s in (1, 2):
    for _b in sorted({1, _s}):
        _add('zero_insert_s%d_beyond%d' % (_s, _b), 'zero_insert', 'stride %d, H1 / W1 %d beyond (Ho - 1) s + 1, a K = 6 slice inside a padded buffer' % (_s, _b),
             _zero_insert(_s, _b),
             promise=lambda kw, s=_s, b=_b: kw['stride'] == s and kw['up'].H == (kw['dy'].H - 1) * s + 1 + b and kw['up'].W == (kw['dy'].W - 1) * s + 1 + b
             and kw['up'].C == kw['dy'].C == 6 and kw['up'].ld == 32 and kw['up'].coff == 4 and bool((kw['up'].t != 0).all()))


def _channel_sum(P, C):
    def build():
        g = _gen(120 + P + C)
        dy = torch.randn(1, 1, P, C, generator=g)
        dy[0, 0, :, 0] = 1e4 * (1 - 2 * (torch.arange(P) % 2).float()) + torch.randn(P, generator=g)      # +-1e4 alternating + O(1)
        return collections.OrderedDict(dy=ops.View(dy), out=torch.full((C,), SENTINEL), ws=None)
    return build


def _promise_channel_sum(kw):
    """Channel 0 alternates in sign at |.| ~ 1e4, so its sum cancels to O(sqrt(P)); C is no multiple of 4 (scalar loads) and leaves a
    partial 64-channel block; the slice count follows the restated arithmetic."""
    dy = kw['dy']
    c0 = dense(dy).reshape(-1, dy.C)[:, 0].double()
    assert bool(((c0.abs() - 1e4).abs() < 10).all()) and bool((c0[:-1] * c0[1:] < 0).all())
    if c0.numel() > 1:
        assert float(c0.sum().abs()) < 2e4 and float(c0.abs().sum()) > 1e4 * (c0.numel() - 1)
    assert dy.C % 4 != 0 and dy.C % 64 != 0
    _promise_slices()(kw)


for _P in (1, 5, 257):
    for _C in (1, 63, 65):
        _add('channel_sum_P%d_C%d' % (_P, _C), 'channel_sum', 'P = %d, C = %d (scalar loads, a partial 64-channel block), a channel of alternating +-1e4' % (_P, _C),
             _channel_sum(_P, _C), promise=_promise_channel_sum)


def _sgd(n, first, wd, mu):
    def build():
        g = _gen(130 + n)
        return collections.OrderedDict(param=torch.randn(n, generator=g), grad=torch.randn(n, generator=g), velocity=torch.randn(n, generator=g),
                                       lr=0.01, momentum=mu, weight_decay=wd, first_step=first)
    return build


def _ema(n, step):
    def build():
        g = _gen(140 + n)
        return collections.OrderedDict(shadow=torch.randn(n, generator=g), param=torch.randn(n, generator=g), step=step, ema_decay=0.9998)
    return build


for _i, _n in enumerate((1, 255, 256, 257)):
    _add('sgd_n%d' % _n, 'sgd_momentum', 'n = %d (the 256-thread block edge); %s step, weight_decay %s, momentum %s'
         % (_n, 'first' if _i & 1 else 'later', 0.0 if _i & 2 else 0.0005, 0.0 if _i == 0 else 0.9),
         _sgd(_n, bool(_i & 1), 0.0 if _i & 2 else 0.0005, 0.0 if _i == 0 else 0.9),
         promise=lambda kw, n=_n, i=_i: kw['param'].numel() == kw['grad'].numel() == kw['velocity'].numel() == n and kw['first_step'] == bool(i & 1)
         and (kw['weight_decay'] == 0.0) == bool(i & 2) and (kw['momentum'] == 0.0) == (i == 0) and bool((kw['velocity'] != 0).all()))
    _add('ema_n%d' % _n, 'ema_update', 'n = %d; step %d: decay (1 + step) / (10 + step) below ema_decay' % (_n, (0, 1000)[_i & 1]), _ema(_n, (0, 1000)[_i & 1]),
         promise=lambda kw, n=_n, i=_i: kw['shadow'].numel() == kw['param'].numel() == n and kw['step'] == (0, 1000)[i & 1]
         and (1 + kw['step']) / (10 + kw['step']) < kw['ema_decay'])
# the four sgd cases between them: a first and a later step, weight_decay = 0, momentum = 0
assert {(CASES['sgd_n%d' % n].build()['first_step']) for n in (1, 255, 256, 257)} == {False, True}


# -- pooling ----------------------------------------------------------------------------------------------------------------------
PATTERNS = ('constant', 'rising h', 'falling h', 'rising w', 'falling w', 'tie two apart')


def pattern_maps(H, W, C, g):
    """[6, H, W, C]: one image per PATTERNS entry (+ a per-channel offset): a constant map (every window one big tie: the first
    position wins), ramps rising / falling along each axis (the maximum sits in the last / first row or column of every window, with
    ties along the other axis), and integer noise with a tie placed two pixels apart."""
    hh = torch.arange(H, dtype=torch.float32).view(H, 1, 1).expand(H, W, C)
    ww = torch.arange(W, dtype=torch.float32).view(1, W, 1).expand(H, W, C)
    noise = torch.randint(-2, 3, (H, W, C), generator=g).float()
    h0, w0 = min(2, H - 1), min(2, W - 1)
    noise[h0, w0, :] = 9.0
    noise[h0, min(w0 + 2, W - 1), :] = 9.0
    x = torch.stack([torch.full((H, W, C), 0.25), hh, -hh, ww, -ww, noise])
    return x + torch.arange(C, dtype=torch.float32).view(1, 1, 1, C)


def first_last_argmax(x, k, stride, pad):
    """Per window of x [N, H, W, C]: (first, last) flat position of the maximum in scan order."""
    N, H, W, C = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (pad, pad, pad, pad), value=-math.inf)
    cols = F.unfold(xp, k, stride=stride).view(N, C, k * k, -1)
    first = cols.argmax(dim=2)
    last = k * k - 1 - cols.flip(2).argmax(dim=2)
    return first, last


def _promise_ties(ks, stride, pad=None):
    """For every window size of `ks`: on the constant image (image 0 of pattern_maps) EVERY window with more than one pixel inside the
    map is a tie -- its first and its last maximum differ --, every window with a single pixel is not; on the falling ramps the first maximum of
    every window is its first pixel inside the map, on the rising ramps the last maximum is its last."""
    def promise(kw):
        x = dense(kw['x'])
        N, H, W, C = x.shape
        for k in ks:
            p = k // 2 if pad is None else pad
            first, last = first_last_argmax(x, k, stride, p)                           # [N, C, L]
            inside = F.unfold(F.pad(torch.ones(1, 1, H, W), (p, p, p, p)), k, stride=stride).sum(dim=1).view(-1)      # pixels of the map per window
            tied = first[0] != last[0]                                                  # [C, L]
            assert bool((tied == (inside > 1).view(1, -1)).all()), 'constant image, window %d: tied windows %s, windows with > 1 pixel %s' % (k, tied[0], inside)
            if H * W > 1:
                assert bool(tied.any())
            # falling ramps: the first maximum is the window's first pixel inside the map; rising ramps: the last one is its last
            assert torch.equal(first[2], first[0]) and torch.equal(first[4], first[0])
            assert torch.equal(last[1], last[0]) and torch.equal(last[3], last[0])
    return promise


def _maxpool(H, W):
    def build():
        x = pattern_maps(H, W, 4, _gen(150 + H * 8 + W))
        return collections.OrderedDict(x=wide(x, 12), y=out_like((6, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 4), True, 16))
    return build


def _maxpool_bwd(H, W):
    def build():
        g = _gen(160 + H * 8 + W)
        x = pattern_maps(H, W, 3, g)
        dy = torch.randn(6, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 3, generator=g)
        return collections.OrderedDict(x=wide(x, 13), dy=wide(dy, 9, 2), dx=out_like((6, H, W, 3), True, 12))
    return build


for _H in (1, 2, 3, 4, 5):
    for _W in (1, 2, 3, 4, 5):
        _add('maxpool_%dx%d' % (_H, _W), 'maxpool3x3s2', '%d x %d, C = 4: constant map and the four ramps' % (_H, _W), _maxpool(_H, _W),
             promise=_promise_ties((3,), 2, 1))
        _add('maxpool_bwd_%dx%d' % (_H, _W), 'maxpool3x3s2_bwd', '%d x %d, C = 3: every window of the constant map is a tie, the first position wins' % (_H, _W),
             _maxpool_bwd(_H, _W), promise=_promise_ties((3,), 2, 1))


def _spp(H, W):
    def build():
        x = pattern_maps(H, W, 8, _gen(170 + H * 16 + W))
        shape = (6, H, W, 8)
        return collections.OrderedDict(x=wide(x, 12), y5=out_like(shape, True, 16), y9=out_like(shape, True, 16), y13=out_like(shape, True, 16))
    return build


def _spp_bwd(H, W, C, patterns=True):
    def build():
        g = _gen(180 + H * 16 + W + C)
        x = pattern_maps(H, W, C, g) if patterns else torch.randint(-3, 4, (1, H, W, C), generator=g).float()
        N = x.shape[0]
        dy = torch.randn(N, H, W, 4 * C, generator=g)
        return collections.OrderedDict(x=wide(x, 12), dy=wide(dy, 8), dx=out_like((N, H, W, C), True, 16), ws=None)
    return build


for _H, _W in ((1, 1), (1, 7), (3, 3), (4, 9), (6, 6), (7, 7), (13, 13)):
    _add('spp_%dx%d' % (_H, _W), 'spp', '%d x %d: a map smaller than the windows; constant map, ramps, a tie two pixels apart' % (_H, _W), _spp(_H, _W),
         promise=_promise_ties((5, 9, 13), 1))
    for _C in (1, 5):
        _add('spp_bwd_%dx%d_C%d' % (_H, _W, _C), 'spp_bwd', '%d x %d, C = %d (a partial group of SPP_CG): the nested 5 -> 9 -> 13 composition on ties' % (_H, _W, _C),
             _spp_bwd(_H, _W, _C), promise=_promise_ties((5, 9, 13), 1))
_add('spp_bwd_37x37_fused', 'spp_bwd', '37 x 37, C = 4, N = 1: the last geometry of the fused kernel', _spp_bwd(37, 37, 4, False),
     promise=lambda kw: spp_bwd_fused(1, 37, 37))
_add('spp_bwd_38x38_four_launch', 'spp_bwd', '38 x 38, C = 4, N = 1: the first geometry of the four-launch form', _spp_bwd(38, 38, 4, False),
     promise=lambda kw: not spp_bwd_fused(1, 38, 38))


def _dropblock_mask(shape, keep, seed):
    def build():
        return collections.OrderedDict(mask=torch.full(shape, SENTINEL), scale=torch.full((1,), SENTINEL), keep_prob=keep, seed=seed)
    return build


_add('dropblock_mask_keep1', 'dropblock_mask', 'keep_prob = 1: the mask is all ones and the scale exactly 1', _dropblock_mask((1, 3, 5, 4), 1.0, 11),
     promise=lambda kw: bool((dropblock_mask_reference(1, 3, 5, 4, 1.0, 11) == 1).all()))
_add('dropblock_mask_3x1', 'dropblock_mask', 'H = 3, W = 1: every window hangs over both side edges', _dropblock_mask((2, 3, 1, 8), 0.6, 12),
     promise=lambda kw: tuple(kw['mask'].shape[1:3]) == (3, 1) and dropblock_tiled(*kw['mask'].shape)
     and 0 < float(dropblock_mask_reference(2, 3, 1, 8, 0.6, 12).sum()) < kw['mask'].numel())
_add('dropblock_mask_W340', 'dropblock_mask', 'W = 340, H = 3, C = 4: the first width of the non-tiled kernel', _dropblock_mask((1, 3, 340, 4), 0.9, 13),
     promise=lambda kw: not dropblock_tiled(1, 3, 340, 4) and dropblock_tiled(1, 3, 339, 4))


# -- contractions --------------------------------------------------------------------------------------------------------------
# The shape tables the suite already has, each call judged per element.  Keys of kw that start with '_' are not arguments of the
# call: '_w_krsc' is the fp32 master behind operand planes (the replay looks it up through a stub of the TrainStep's weight cache).
BACKWARD_CASES = [  # N, H, W, C, K, R, stride: head layer shapes at small maps + ragged ones (tests/test_gpu_backward.py runs the same list)
    (2, 19, 19, 512, 1024, 3, 1), (2, 19, 19, 1024, 512, 1, 1), (2, 19, 19, 1024, 258, 1, 1), (1, 38, 38, 256, 512, 3, 1),
    (2, 12, 12, 128, 258, 1, 1), (3, 7, 5, 64, 96, 3, 1), (1, 9, 9, 32, 40, 3, 1), (2, 6, 6, 96, 255, 1, 1), (1, 1, 1, 64, 64, 1, 1),
    (2, 11, 3, 160, 33, 3, 1), (5, 2, 2, 32, 130, 3, 1),
]
NINE_TAP_SHAPES = [(2, 7, 10, 32, 72), (1, 1, 5, 64, 128), (3, 6, 1, 32, 40), (2, 19, 19, 96, 260), (8, 38, 38, 64, 128)]      # test_wgrad_nine_tap_kernel_edge_shapes
IMAGE_SCALES = [1.0, 30.0, 0.02, 5.0, 1.0, 2.0, 0.5, 1.0]
DGRAD_FAMILIES = ('fp32', 'bf16x3', 'f16x2', 'f16x2_slab', 'f16x2_tall', 'ws', 'kparity', 'small')      # general geometry, plain (not pre-split) input


def _tag(shape):
    return 'x'.join(str(v) for v in shape)


def _planes_stub(K):
    return (torch.zeros(2, dtype=torch.int16), torch.ones(K))


def _prep_planes(o, kw):
    w = kw.get('_w_krsc', kw.get('w_krsc'))
    kw['w_f16'] = o.split_weights_f16x2(w, torch.ones(w.shape[0], device=w.device))


def _wgrad(shape, f16, x_slice=None, dy_slice=None, seed=0):
    def build():
        N, H, W, C, K, R, stride = shape
        pad = (R - 1) // 2
        g = _gen(2000 + seed)
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        x = torch.randn(N, H, W, C, generator=g) * torch.tensor(IMAGE_SCALES[:N]).view(N, 1, 1, 1)
        dy = torch.randn(N, Ho, Wo, K, generator=g) * torch.exp(torch.randn(N, Ho, Wo, K, generator=g) * 2.0) * 1e-3
        xv = ops.View(x) if x_slice is None else wide(x, x_slice[1], x_slice[0])
        dyv = ops.View(dy) if dy_slice is None else wide(dy, dy_slice[1], dy_slice[0])
        return collections.OrderedDict(x=xv, dy=dyv, dw_krsc=torch.full((K, R, R, C), SENTINEL), stride=stride, pad=pad, ws=None,
                                       amax_x=ops.amax_slots(x) if f16 else None, amax_dy=ops.amax_slots(dy) if f16 else None)
    return build


def _promise_wgrad(shape, f16, nine, x_slice, dy_slice, env=None):
    """The call has the geometry, the operand kind, the slices and the kernel form (nine taps / one tap per workgroup) its name says;
    the per-image maxima in the slots are the operands' own."""
    def promise(kw):
        N, H, W, C, K, R, stride = shape
        x, dy = kw['x'], kw['dy']
        pad = kw['pad']
        assert (x.N, x.H, x.W, x.C) == (N, H, W, C) and (dy.N, dy.H, dy.W, dy.C) == (N,) + tuple(ops.conv_out_hw(H, W, R, R, stride, pad)) + (K,)
        assert tuple(kw['dw_krsc'].shape) == (K, R, R, C) and kw['stride'] == stride
        assert (kw['amax_x'] is not None) == f16 == (kw['amax_dy'] is not None)
        if f16:
            assert torch.equal(kw['amax_x'].view(N, -1).amax(1), dense(x).abs().reshape(N, -1).amax(1))
            assert torch.equal(kw['amax_dy'].view(N, -1).amax(1), dense(dy).abs().reshape(N, -1).amax(1))
        assert wgrad_nine_tap(C, R, R, stride, pad, f16, env) == nine
        for v, s in ((x, x_slice), (dy, dy_slice)):
            assert (v.coff, v.ld - v.C) == ((0, 0) if s is None else s) and (s is None or v.ld % 4 == 0)
    return promise


def _add_wgrad(tag, shape, why, x_slice=None, dy_slice=None, promise=None):
    N, H, W, C, K, R, stride = shape
    pad = (R - 1) // 2
    seed = sum(shape)
    nine = wgrad_nine_tap(C, R, R, stride, pad, True)
    also = [promise] if promise is not None else []
    _add('wgrad_%s_bf16x3' % tag, 'conv2d_wgrad', why + '; bf16x3', _wgrad(shape, False, x_slice, dy_slice, seed),
         promise=_all(_promise_wgrad(shape, False, False, x_slice, dy_slice), *also))
    _add('wgrad_%s_f16x2' % tag, 'conv2d_wgrad', why + '; f16x2 with tracked maxima' + (', nine taps per workgroup' if nine else ''),
         _wgrad(shape, True, x_slice, dy_slice, seed), promise=_all(_promise_wgrad(shape, True, nine, x_slice, dy_slice), *also))
    if nine:        # (elsewhere the switch selects nothing: the same launch)
        env = {'PPY_WGRAD9': '0'}
        _add('wgrad_%s_f16x2_one_tap' % tag, 'conv2d_wgrad', why + '; f16x2, PPY_WGRAD9=0: one tap per workgroup', _wgrad(shape, True, x_slice, dy_slice, seed),
             env=env, promise=_all(_promise_wgrad(shape, True, False, x_slice, dy_slice, env), *also))


for _c in BACKWARD_CASES:
    _add_wgrad(_tag(_c), _c, 'backward table N%d %dx%d C%d K%d R%d s%d' % _c)
for _c in NINE_TAP_SHAPES:
    _add_wgrad('nine_' + _tag(_c), _c + (3, 1), 'nine-tap edge shape N%d %dx%d C%d K%d (W %% 4, one-row / one-column maps, K tail), slices' % _c,
               x_slice=(16, 32), dy_slice=(4, (_c[4] + 3) // 4 * 4 - _c[4] + 8), promise=lambda kw: kw['x'].C % 32 == 0 and kw['x'].ld > kw['x'].C and kw['dy'].ld > kw['dy'].C)
assert {(c[2] % 4 != 0, c[1] == 1, c[2] == 1, c[4] % 64 != 0) for c in NINE_TAP_SHAPES} >= {(True, False, False, True), (True, True, False, False), (True, False, True, True)}
_add_wgrad('strided_sliced', (2, 13, 10, 64, 48, 3, 2), 'stride 2, x and dy channel slices of wider buffers', x_slice=(16, 32), dy_slice=(8, 16),
           promise=lambda kw: kw['stride'] == 2 and kw['x'].ld > kw['x'].C and kw['dy'].ld > kw['dy'].C)


def _promise_1x1_map(kw):
    x, dy = dense(kw['x']).double(), dense(kw['dy']).double()
    assert x.shape[1:3] == (1, 1) and kw['dw_krsc'].shape[1:3] == (3, 3) and bool((dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1]) != 0).all())


_add_wgrad('1x1map', (2, 1, 1, 32, 8, 3, 1), '3 x 3 on a 1 x 1 map: the eight off-centre taps are exactly 0', promise=_promise_1x1_map)
_add_wgrad('s2_evenH', (2, 8, 6, 32, 16, 3, 2), 'stride 2 on an even H / W: tap 2 of the last output row ends on the last input row, the bottom / right padding is never read',
           promise=lambda kw: kw['stride'] == 2 and kw['x'].H % 2 == 0 and kw['x'].W % 2 == 0 and 2 * (kw['dy'].H - 1) + 2 - kw['pad'] == kw['x'].H - 1
           and 2 * (kw['dy'].W - 1) + 2 - kw['pad'] == kw['x'].W - 1)
_add_wgrad('stem_C3', (2, 9, 8, 3, 32, 3, 2), 'C = 3: the stem\'s weight gradient (x a slice of a 4-channel buffer)', x_slice=(0, 1),
           promise=lambda kw: kw['x'].C == 3 and kw['x'].ld == 4)


def _dgrad(shape, f16, cfg=-1, splitk=0, prepared=False, seed=0):
    def build():
        N, H, W, C, K, R, _ = shape
        pad = (R - 1) // 2
        g = _gen(2100 + seed)
        w = torch.randn(K, R, R, C, generator=g) * (1.0 / (C * R * R)) ** 0.5
        dy = torch.randn(N, H, W, K, generator=g) * torch.tensor(IMAGE_SCALES[:N]).view(N, 1, 1, 1) * 1e-3
        Kp = (K + 3) // 4 * 4
        dyv = wide(dy, Kp - K + 8, 4) if K % 32 else ops.View(dy)        # (a K that is padded to 32 is copied: dy_ld % 4 == 0, 16-byte aligned)
        dx = out_like((N, H, W, C), True, 16)
        am = ops.amax_slots(dy) if f16 or prepared else None
        if prepared:
            Kp32 = (K + 31) // 32 * 32
            prep = dict(w=w, dgrad=True, dg_planes=torch.zeros(1, dtype=torch.int16), dg_wt=torch.zeros(C, R, R, Kp32))
            return collections.OrderedDict(dy=dyv, prep=prep, dx=dx, pad=pad, ones=torch.ones(C), zeros=torch.zeros(C), ws=None, cfg=cfg, splitk=splitk,
                                           amax_dy=am)
        return collections.OrderedDict(dy=dyv, w_krsc=w, dx=dx, stride=1, pad=pad, ws=None, cfg=cfg, splitk=splitk, amax_dy=am)
    return build


def _prep_table(o, kw):
    ent = dict(w=kw['prep']['w'], dgrad=True)
    tab = o.WeightPrepTable([ent])
    tab.build()
    kw['prep'] = ent
    kw['_table'] = tab


DGRAD_SHAPES = [(_tag(c), c) for c in BACKWARD_CASES if c[6] == 1] + [
    ('1x1map', (2, 1, 1, 32, 32, 3, 1)), ('1xWmap', (2, 1, 7, 32, 40, 3, 1)), ('Hx1map', (2, 6, 1, 32, 40, 3, 1))]
def _promise_dgrad(shape, f16, cfg=-1, splitk=0):
    """Geometry, operand kind, tile id and split as named; a K that is no multiple of 32 comes as a 16-byte aligned slice (the entry
    point copies it into a padded buffer), dx is a slice with sentinels."""
    def promise(kw):
        N, H, W, C, K, R, _ = shape
        dy, dx = kw['dy'], kw['dx']
        w = kw['prep']['w'] if 'prep' in kw else kw['w_krsc']
        assert (dy.N, dy.H, dy.W, dy.C) == (N, H, W, K) and (dx.N, dx.H, dx.W, dx.C) == (N, H, W, C) and tuple(w.shape) == (K, R, R, C)
        assert kw['pad'] == (R - 1) // 2 and (kw['cfg'], kw['splitk']) == (cfg, splitk) and (kw['amax_dy'] is not None) == f16
        assert (dy.coff == 4 and dy.ld % 4 == 0 and dy.ld > K) if K % 32 else (dy.coff == 0 and dy.ld == K)
        assert dx.coff == 4 and bool((dx.t == SENTINEL).all())
        if cfg >= 0:
            d = ops.conv_cfg(cfg)
            assert d.family in DGRAD_FAMILIES and (d.operands == 'f16x2') == f16 and (splitk == 1 or d.splitk_mode != 'none')
    return promise


for _t, _c in DGRAD_SHAPES:
    _why = 'N%d %dx%d C%d K%d R%d' % _c[:6] + (' (K padded to 32 through a copy)' if _c[4] % 32 else '')
    _add('dgrad_%s_bf16x3' % _t, 'conv2d_dgrad', _why + '; the default choice, bf16x3', _dgrad(_c, False, seed=sum(_c)), promise=_promise_dgrad(_c, False))
    _add('dgrad_%s_f16x2' % _t, 'conv2d_dgrad', _why + '; the default choice, f16x2 with tracked maxima', _dgrad(_c, True, seed=sum(_c)),
         promise=_promise_dgrad(_c, True))
    _add('dgrad_prepared_%s' % _t, 'conv2d_dgrad_prepared', _why + '; on the planes of a prepared-weight table', _dgrad(_c, True, prepared=True, seed=sum(_c)),
         prep=_prep_table, promise=_all(_promise_dgrad(_c, True), lambda kw: kw['prep']['w'].shape[3] % 32 == 0))
_seen = set()
for _cfg in ops.conv_cfgs():
    if _cfg.family in DGRAD_FAMILIES and _cfg.family not in _seen:
        _seen.add(_cfg.family)
        for _sk in (1, 3) if _cfg.splitk_mode != 'none' else (1,):
            _add('dgrad_family_%s_splitk%d' % (_cfg.family, _sk), 'conv2d_dgrad', 'N3 7x5 C64 K96 R3 on id %d (family %s), split-K %d' % (_cfg.id, _cfg.family, _sk),
                 _dgrad((3, 7, 5, 64, 96, 3, 1), _cfg.operands == 'f16x2', _cfg.id, _sk, seed=_cfg.id),
                 promise=_promise_dgrad((3, 7, 5, 64, 96, 3, 1), _cfg.operands == 'f16x2', _cfg.id, _sk))
assert _seen == set(DGRAD_FAMILIES)


# conv2d_train_fwd: the table of test_batchnorm_statistics_from_the_convolution_epilogue
def _train_fwd_table():
    wsf, pf, sf = ops.ws_first_cfg(), ops.patch_first_cfg(), ops.stream_first_cfg()
    return [((2, 19, 19, 64, 128, 3, 1), (41, 44, 47, 48, 51, 66, 70, wsf, wsf + 2)), ((3, 13, 11, 96, 258, 1, 1), (41, 44, wsf + 1)),
            ((8, 76, 76, 32, 64, 3, 1), (44, wsf + 3, pf)), ((5, 9, 7, 160, 40, 3, 2), (48, wsf)), ((1, 4, 4, 32, 32, 1, 1), (41,)),
            ((3, 21, 37, 32, 32, 3, 1), (pf, 85)), ((3, 24, 20, 64, 256, 1, 1), (sf, sf + 1, 88)), ((2, 9, 7, 128, 128, 1, 1), (sf,))]


def _conv_inputs(shape, g):
    N, H, W, C, K, R, stride = shape
    x = torch.randn(N, H, W, C, generator=g) * torch.exp(1.5 * torch.randn(N, 1, 1, 1, generator=g)) + 0.3
    w = torch.randn(K, R, R, C, generator=g) * (1.0 / (R * R * C) ** 0.5)
    return x, w


def _train_fwd(shape, cfg):
    def build():
        N, H, W, C, K, R, stride = shape
        pad = (R - 1) // 2
        g = _gen(2200 + sum(shape))
        x, w = _conv_inputs(shape, g)
        Ho, Wo = ops.conv_out_hw(H, W, R, R, stride, pad)
        part = torch.full((ops.conv2d_bn_partials_bytes(N * Ho * Wo, K) // 4,), SENTINEL)
        return collections.OrderedDict(x=ops.View(x), w_krsc=w, w_f16=_planes_stub(K), bias=torch.randn(K, generator=g), y=out_like((N, Ho, Wo, K), K % 4 == 0, 16),
                                       stride=stride, pad=pad, cfg=cfg, amax_in=ops.amax_slots(x), partials=part)
    return build


def _promise_train_fwd(shape, cfg):
    """The id is an f16x2 tile whose epilogue writes the BatchNorm partials (or the twin of one), the partials buffer has the size the
    library asks for, and y is a slice wherever K allows 16-byte stores."""
    def promise(kw):
        N, H, W, C, K, R, stride = shape
        d = ops.conv_cfg(cfg)
        assert d.operands == 'f16x2' and (d.bn_stats or d.stats_twin >= 0) and kw['cfg'] == cfg
        x, y = kw['x'], kw['y']
        assert (x.N, x.H, x.W, x.C) == (N, H, W, C) and (y.H, y.W) == tuple(ops.conv_out_hw(H, W, R, R, stride, kw['pad'])) and y.C == K
        assert kw['partials'].numel() * 4 == ops.conv2d_bn_partials_bytes(y.N * y.H * y.W, K) and (y.coff == 4) == (K % 4 == 0)
        assert N * H * W * C <= 8 * 76 * 76 * 32
    return promise


for _c, _cfgs in _train_fwd_table():
    for _cfg in _cfgs:
        _add('train_fwd_%s_cfg%d' % (_tag(_c), _cfg), 'conv2d_train_fwd', 'N%d %dx%d C%d K%d R%d s%d' % _c + ' on id %d (family %s): y and the BatchNorm partials'
             % (_cfg, ops.conv_cfg(_cfg).family), _train_fwd(_c, _cfg), prep=_prep_planes, promise=_promise_train_fwd(_c, _cfg))

# conv1x1_stats / conv1x1_bn_apply: the table of test_frozen_1x1_layers_without_the_raw_tensor (N, H, W, C, K, act, residual, variant, y as a slice)
FROZEN_1X1 = [(3, 24, 20, 64, 256, 'relu', True, 0, False), (2, 9, 7, 128, 128, None, False, 0, False), (2, 19, 19, 64, 64, 'leaky', False, 1, True),
              (4, 13, 11, 128, 512, 'relu', True, 1, False), (8, 38, 38, 64, 256, 'relu', True, 0, False)]


def _conv1x1(row, apply):
    def build():
        N, H, W, C, K, act, use_res, variant, wide_y = row
        g = _gen(2300 + N * H + K)
        x, w = _conv_inputs((N, H, W, C, K, 1, 1), g)
        bias = torch.zeros(K)
        am = ops.amax_slots(x)
        if not apply:
            part = torch.full((ops.conv2d_bn_partials_bytes(N * H * W, K) // 4,), SENTINEL)
            return collections.OrderedDict(x=ops.View(x), w_f16=_planes_stub(K), bias=bias, Kout=K, variant=variant, amax_in=am, partials=part, _w_krsc=w)
        yy = (x.double().reshape(-1, C) @ w.double().reshape(K, C).t())
        mean, invstd = _stats_of(yy.view(N, H, W, K))
        gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
        res = ops.View(torch.randn(N, H, W, K, generator=g)) if use_res else None
        return collections.OrderedDict(x=ops.View(x), w_f16=_planes_stub(K), bias=bias, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
                                       y=out_like((N, H, W, K), wide_y, K), act=act, residual=res, variant=variant, amax_in=am,
                                       amax_out=ops.amax_slots(N=N), _w_krsc=w)
    return build


for _r in FROZEN_1X1:
    _t = 'N%d_%dx%d_C%d_K%d' % _r[:5]
    _add('conv1x1_stats_' + _t, 'conv1x1_stats', 'frozen 1x1 layer, variant %d: the partials without the raw tensor' % _r[7], _conv1x1(_r, False), prep=_prep_planes,
         promise=lambda kw, r=_r: (kw['x'].N, kw['x'].H, kw['x'].W, kw['x'].C, kw['Kout'], kw['variant']) == r[:5] + (r[7],) and r[3] in (64, 128)
         and kw['partials'].numel() * 4 == ops.conv2d_bn_partials_bytes(r[0] * r[1] * r[2], r[4]))
    _add('conv1x1_bn_apply_' + _t, 'conv1x1_bn_apply', 'frozen 1x1 layer, variant %d, act %s, residual %s%s' % (_r[7], _r[5], _r[6], ', y a slice' if _r[8] else ''),
         _conv1x1(_r, True), prep=_prep_planes,
         promise=lambda kw, r=_r: (kw['x'].N, kw['x'].H, kw['x'].W, kw['x'].C, kw['y'].C, kw['variant']) == r[:5] + (r[7],) and kw['act'] == r[5]
         and (kw['residual'] is not None) == r[6] and (kw['y'].ld > kw['y'].C) == r[8])


def _conv_bn_act():
    shape = (2, 7, 5, 32, 40, 3, 1)
    g = _gen(2400)
    x, w = _conv_inputs(shape, g)
    K = 40
    ws = torch.zeros(max(1, ops.conv2d_workspace_bytes(2, 7, 5, 32, K, 3, 3, 1, 1) // 4))      # (the library's choice may split the reduction)
    return collections.OrderedDict(x=wide(x, 12), w_krsc=w, scale=torch.rand(K, generator=g) + 0.5, shift=torch.randn(K, generator=g), y=out_like((2, 7, 5, K), True, 16),
                                   stride=1, pad=1, act='leaky', residual=wide(torch.randn(2, 7, 5, K, generator=g), 8), ws=ws,
                                   amax_out=ops.amax_slots(N=2))


_add('conv_bn_act_small', 'conv2d_bn_act', 'N2 7x5 C32 K40 R3: the library\'s own choice on fp32 operands, slices, shortcut, leaky, tracked maximum', _conv_bn_act,
     promise=_all(_promise_pitches('x', 'y'), lambda kw: kw['residual'] is not None and kw['act'] == 'leaky' and kw['amax_out'] is not None
                  and kw['ws'].numel() * 4 >= ops.conv2d_workspace_bytes(2, 7, 5, 32, 40, 3, 3, 1, 1)))
