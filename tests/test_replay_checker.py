"""The launch-level oracle of tests/launch_replay.py is neither vacuous nor flaky: with torch float32 on the CPU standing in for the
kernels, correct convolutions, data and weight gradients at the training step's reduction lengths pass, and each injected defect
-- the size of the bugs a tiled kernel makes -- fails.  No GPU: the checkers run on whatever device the tensors live on."""
import pytest
import torch
import torch.nn.functional as F

import launch_replay as lr
from ppyolo_hip import ops


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _conv_case(N, H, C, K, R, stride, seed, ld_extra=0, coff=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, H, C, generator=g)
    w = torch.randn(K, R, R, C, generator=g) / (R * R * C) ** 0.5
    bias = torch.randn(K, generator=g) * 0.1
    pad = (R - 1) // 2
    Ho = (H + 2 * pad - R) // stride + 1
    ybuf = torch.randn(N, Ho, Ho, coff + K + ld_extra, generator=g)
    return x, w, bias, pad, ybuf


def _run_conv(inject=None, N=1, H=12, C=1024, K=80, R=3, stride=1, seed=0):
    """conv2d_bn_act (scale 1, shift = bias) with F.conv2d in fp32 as the implementation; `inject(y_nhwc_slice, ref_fp32)` mutates
    the result in place before it lands, or gets the whole buffer (write past the slice)."""
    x, w, bias, pad, ybuf = _conv_case(N, H, C, K, R, stride, seed, ld_extra=8, coff=16)
    xv, yv = ops.View(x), ops.View(ybuf, 16, K)
    one = torch.ones(K)

    def impl():
        y = _nhwc(F.conv2d(_nchw(x), _nchw(w), bias, stride=stride, padding=pad))
        if inject is not None:
            inject(y, ybuf, x, w)
        ybuf[..., 16:16 + K] = y

    rep = lr.Replay(ops)
    rep.run('conv2d_bn_act', rep.bind(ops.conv2d_bn_act, xv, w, one, bias, yv, stride, pad, None, cfg=-1), impl)
    return rep


def _assert_pass(rep):
    assert not rep.failures, rep.report()
    assert rep.census and rep.census[-1]['checks']


def _assert_fail(rep, what=None):
    assert rep.failures, 'the defect went unnoticed: ' + rep.report()
    if what is not None:
        assert any(what in f['what'] for f in rep.failures), rep.report()


def test_fp32_convolution_passes_at_k_9216():
    rep = _run_conv()
    _assert_pass(rep)
    print(rep.report('fp32 conv k=9216'))


def test_strided_convolution_passes():
    _assert_pass(_run_conv(C=256, K=64, stride=2, H=13))


def test_dropped_tap_at_one_pixel_fails():
    def drop(y, ybuf, x, w):          # output pixel (0, 5, 7): tap (r, s) = (0, 0) reads x[0, 4, 6]
        y[0, 5, 7] -= x[0, 4, 6] @ w[:, 0, 0, :].t()
    _assert_fail(_run_conv(drop), 'conv')


def test_dropped_32_channel_chunk_fails_at_the_largest_k():
    def drop(y, ybuf, x, w):          # element (0, 3, 3, 11): channels 512..543 of tap (1, 1) missing
        y[0, 3, 3, 11] -= float(x[0, 3, 3, 512:544] @ w[11, 1, 1, 512:544])
    _assert_fail(_run_conv(drop), 'conv')


def test_one_element_off_by_1e4_relative_fails():
    def off(y, ybuf, x, w):
        i = int(y.abs().argmax())
        y.view(-1)[i] *= 1 + 1e-4
    _assert_fail(_run_conv(off), 'conv')


def test_swapped_channel_of_the_k_tail_fails():
    def swap(y, ybuf, x, w):          # K = 80: channels 64..79 are the tail of a 64-wide tile
        y[..., [70, 71]] = y[..., [71, 70]]
    _assert_fail(_run_conv(swap), 'conv')


def test_write_one_channel_past_the_slice_fails():
    def spill(y, ybuf, x, w):
        ybuf[..., 16 + 80] = 0.0
    _assert_fail(_run_conv(spill), 'outside')


def test_transposed_convolution_passes():
    """conv2d_dgrad with F.conv_transpose2d as the implementation (k = 9 * 1024)."""
    g = torch.Generator().manual_seed(3)
    N, H, C, K = 1, 10, 64, 1024
    dy = torch.randn(N, H, H, K, generator=g)
    w = torch.randn(K, 3, 3, C, generator=g) / 96.0
    dx = torch.zeros(N, H, H, C)

    def impl():
        dx.copy_(_nhwc(F.conv_transpose2d(_nchw(dy), _nchw(w), padding=1)))
    rep = lr.Replay(ops)
    rep.run('conv2d_dgrad', rep.bind(ops.conv2d_dgrad, ops.View(dy), w, ops.View(dx), 1, 1), impl)
    _assert_pass(rep)

    def impl_bad():
        impl()
        dx[0, 4, 4, 9] += 1e-4 * float(dx.abs().max())
    rep = lr.Replay(ops)
    rep.run('conv2d_dgrad', rep.bind(ops.conv2d_dgrad, ops.View(dy), w, ops.View(dx), 1, 1), impl_bad)
    _assert_fail(rep, 'dgrad')


@pytest.mark.parametrize('stride', [1, 2])
def test_weight_gradient_passes_at_k_2080(stride):
    """conv2d_wgrad with torch.nn.grad.conv2d_weight as the implementation; k = N * Ho * Wo = 2080."""
    g = torch.Generator().manual_seed(4)
    N, H, W, C, K = 8, 13 * stride, 20 * stride, 64, 96
    x = torch.randn(N, H, W, C, generator=g)
    dy = torch.randn(N, H // stride, W // stride, K, generator=g)
    dw = torch.zeros(K, 3, 3, C)

    def impl():
        dw.copy_(torch.nn.grad.conv2d_weight(_nchw(x), (K, C, 3, 3), _nchw(dy), stride=stride, padding=1).permute(0, 2, 3, 1))
    rep = lr.Replay(ops)
    args = rep.bind(ops.conv2d_wgrad, ops.View(x), ops.View(dy), dw, stride, 1)
    rep.run('conv2d_wgrad', args, impl)
    _assert_pass(rep)
    assert rep.census[-1]['geom'][:3] == (N, H, W)

    def impl_bad():          # one 32-row chunk of the reduction dropped for one element
        impl()
        P0 = 32 * 7
        xs = F.pad(x, (0, 0, 1, 1, 1, 1))[:, 1:1 + stride * (H // stride):stride, 1:1 + stride * (W // stride):stride, :].reshape(-1, C)
        dw[5, 1, 1, 3] -= float(dy.reshape(-1, K)[P0:P0 + 32, 5] @ xs[P0:P0 + 32, 3])
    rep = lr.Replay(ops)
    rep.run('conv2d_wgrad', args, impl_bad)
    _assert_fail(rep, 'wgrad')


def _bn_stats_args(P=2048, C=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 32, P // 64, C, generator=g) * 3 + 1.5
    mean, invstd = torch.empty(C), torch.empty(C)
    rm, rv = torch.zeros(C), torch.ones(C)
    return x, mean, invstd, rm, rv


def _bn_impl(x, mean, invstd, rm, rv, inv_err=0.0):
    def impl():
        xx = x.reshape(-1, x.shape[-1]).double()
        m, v = xx.mean(0), xx.var(0, unbiased=False)
        mean.copy_(m.float())
        invstd.copy_((1 / (v + 1e-5).sqrt() * (1 + inv_err)).float())
        rm.copy_((0.9 * rm.double() + 0.1 * m).float())
        rv.copy_((0.9 * rv.double() + 0.1 * xx.var(0, unbiased=True)).float())
    return impl


@pytest.mark.parametrize('err,ok', [(0.0, True), (1e-5, False)])
def test_batchnorm_statistics(err, ok):
    x, mean, invstd, rm, rv = _bn_stats_args()
    rep = lr.Replay(ops)
    rep.run('bn_train_stats', rep.bind(ops.bn_train_stats, ops.View(x), 1e-5, 0.1, mean, invstd, rm, rv), _bn_impl(x, mean, invstd, rm, rv, err))
    if ok:
        _assert_pass(rep)
    else:
        _assert_fail(rep, 'invstd')


@pytest.mark.parametrize('under', [False, True])
def test_tracked_maximum_must_not_fall_below_the_output(under):
    g = torch.Generator().manual_seed(6)
    N, C = 2, 32
    x = torch.randn(N, 6, 6, C, generator=g)
    y = torch.empty_like(x)
    mean, invstd = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.1
    amax = torch.zeros(N * ops.AMAX_FLOATS_PER_IMAGE)

    def impl():
        z = (x.double() - mean.double()) * (invstd.double() * gamma.double()) + beta.double()
        y.copy_(torch.where(z > 0, z, 0.1 * z).float())
        m = y.reshape(N, -1).abs().amax(1)
        amax.view(N, -1)[:, 3] = m * (1 - 2 ** -20) if under else m
    rep = lr.Replay(ops)
    rep.run('bn_train_apply', rep.bind(ops.bn_train_apply, ops.View(x), mean, invstd, gamma, beta, ops.View(y), 'leaky', None, amax), impl)
    if under:
        _assert_fail(rep, 'amax')
    else:
        _assert_pass(rep)


def test_allowlist_and_checkers_cover_every_op():
    """Every launch-issuing function of ppyolo_hip/ops.py has a checker, or sits on the allowlist with a reason."""
    import inspect
    names = [n for n, f in vars(ops).items() if not n.startswith('_') and n not in lr.HOST
             and (inspect.isfunction(f) or inspect.isclass(f)) and getattr(f, '__module__', None) == ops.__name__]
    train_ops = set()
    import ppyolo_hip.train as tr
    src = inspect.getsource(tr)
    import re
    train_ops = set(re.findall(r'\bK\.([a-zA-Z_0-9]+)\(', src)) - lr.HOST
    missing = sorted(n for n in train_ops if not hasattr(lr.Replay, 'chk_' + n) and n not in lr.ALLOWLIST)
    assert not missing, 'ops the training step calls without a replay reference: %s' % missing
    assert train_ops <= set(names)
