"""GPU parity of every HIP kernel against the reference-generated goldens and the CPU oracle,
called through the C ABI (ppyolo_hip.ops -> ctypes -> libppyolo_hip.so).

Tolerances: convolutions sum fp32 products in a different order than MKLDNN, so they are
compared at 2e-5 relative to the tensor's magnitude; the DCN gather, the box decode and
Matrix-NMS reproduce the reference arithmetic op for op and are compared (almost) bit-exactly;
NMS keep-indices must be identical."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ppyolo_oracle as orc

pytestmark = pytest.mark.gpu

ACTS = {0: None, 1: 'relu', 2: 'leaky'}


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rel=2e-5, what=''):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= rel * scale, '%s: max abs err %.3e (scale %.3e)' % (what, err, scale)
    return err / scale


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------
def test_conv_units_golden(golden):
    from model.custom_layers import Conv2dUnit
    g = golden('g1_conv_units')
    for i in range(int(g['ncases'])):
        p = 'c%d_' % i
        ci, co, k, s, act, bn, bias = [int(v) for v in g[p + 'meta']]
        u = Conv2dUnit(ci, co, k, stride=s, bias_attr=bool(bias), bn=bn, act=ACTS[act])
        with torch.no_grad():
            u.conv.weight.copy_(T(g[p + 'w']))
            if bias:
                u.conv.bias.copy_(T(g[p + 'b']))
            if bn:
                b = T(g[p + 'bn'])
                u.bn.weight.copy_(b[0]); u.bn.bias.copy_(b[1])
                u.bn.running_mean.copy_(b[2]); u.bn.running_var.copy_(b[3])
        u = u.eval().cuda()
        y = u(T(g[p + 'x']).cuda())
        close(y, T(g[p + 'y']), what='conv unit %d' % i)


NUM_CFGS = 94      # 31 exact-fp32 MFMA configurations + 9 bf16x3 + 9 f16x2 with 2 LDS stages + 9 with 3 + 9 with 4
                   # + 9 + 9 f16x2 with slab reuse (3x3 / stride 1 / pad 1 only) and 2 / 3 stages
                   # + 3 x 3 f16x2 tiles of 192x128 / 192x256 / 96x256 with 2 / 3 / 4 stages (conv_x3.hip)
SLAB0, SLAB1 = 67, 85      # (the parametrisations below are laid out at collection, before there is a library to ask)


def first_cfg(family):
    """First conv cfg id of a family, from the library's descriptors (ops.conv_cfgs)."""
    from ppyolo_hip import ops
    return next(d.id for d in ops.conv_cfgs() if d.family == family)


def test_literal_id_ranges_match_the_descriptors():
    from ppyolo_hip import ops
    assert [d.id for d in ops.conv_cfgs() if d.family == 'f16x2_slab'] == list(range(SLAB0, SLAB1))
    assert first_cfg('stream') == NUM_CFGS


@pytest.mark.parametrize('cfg', range(NUM_CFGS))
@pytest.mark.parametrize('splitk', [1, 3])
def test_conv_every_tile_config(cfg, splitk):
    """Each tile configuration / split-K path, with channel-sliced input & output buffers,
    residual, per-position bias, odd sizes (M and K tails)."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(100 + cfg)
    N, H, W, C, K, R = 2, 13, 11, 64, 200, 3
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) * 0.05
    scale = torch.rand(K, generator=g) + 0.5
    shift = torch.randn(K, generator=g)
    res = torch.randn(N, K, H, W, generator=g)
    posb = torch.randn(1, K, H, W, generator=g)
    ref = F.conv2d(x, w, None, 1, 1) + posb
    ref = F.leaky_relu(ref * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res, 0.1)
    xin = torch.zeros(N, H, W, C + 32).cuda()
    xin[..., 32:] = nhwc(x).cuda()
    yout = torch.full((N, H, W, K + 8), -7.0).cuda()
    rbuf = torch.zeros(N, H, W, K + 4).cuda()
    rbuf[..., 4:] = nhwc(res).cuda()
    ws = torch.empty(max(4, ops.conv2d_workspace_bytes(N, H, W, C, K, R, R, 1, 1, cfg, splitk) // 4)).cuda()
    wk = w.permute(0, 2, 3, 1).contiguous().cuda()
    f16 = cfg >= 40
    wf = ops.split_weights_f16x2(wk, scale.cuda()) if f16 else None
    pb = nhwc(posb).contiguous().cuda()
    amax_out = ops.amax_slots(device='cuda', N=N)
    ops.conv2d_bn_act(ops.View(xin, 32, C), wk, scale.cuda(), shift.cuda(),
                      ops.View(yout, 8, K), 1, 1, 'leaky', residual=ops.View(rbuf, 4, K),
                      posbias=pb, cfg=cfg, splitk=splitk, ws=ws,
                      w_x3=ops.split_weights_bf16x3(wk) if 31 <= cfg < 40 else None, w_f16=wf,
                      amax_in=ops.amax_slots(xin) if f16 else None, amax_out=amax_out,
                      posbias_f16=(pb * (scale.cuda() / wf[1])).contiguous() if f16 else None)
    torch.cuda.synchronize()
    got_amax = amax_out.view(N, -1).amax(dim=1).cpu()
    assert (got_amax - ref.abs().reshape(N, -1).amax(dim=1)).abs().max() <= 1e-3, 'tracked per-image max|y| is off'
    close(nchw(yout[..., 8:]), ref, what='cfg %d split %d' % (cfg, splitk))
    assert torch.all(yout[..., :8] == -7.0), 'wrote outside the output channel slice'


@pytest.mark.parametrize('cfg', list(range(49, 67)) + list(range(88, 94)))
def test_deep_stage_variants_on_short_reductions(cfg):
    """3- and 4-stage f16x2 variants when the reduction has fewer chunks than stages (1, 2, 3 chunks; split-K leaving one
    chunk per split): the unused stage slots are requested as out-of-range dummies and must not leak into the result."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(500 + cfg)
    for C, R, splitk in ((32, 1, 1), (64, 1, 1), (96, 1, 1), (64, 1, 2), (32, 3, 9), (160, 1, 2)):
        N, H, W, K = 2, 17, 9, 72
        x = torch.randn(N, C, H, W, generator=g)
        w = torch.randn(K, C, R, R, generator=g) * 0.1
        sc, sh = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
        ref = F.relu(F.conv2d(x, w, None, 1, (R - 1) // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        y = torch.full((N, H, W, K), 9.0).cuda()
        ws = torch.empty(1 << 20).cuda()
        ops.conv2d_bn_act(ops.View(xd), wk, sc.cuda(), sh.cuda(), ops.View(y), 1, (R - 1) // 2, 'relu', cfg=cfg, splitk=splitk,
                          ws=ws, w_f16=ops.split_weights_f16x2(wk, sc.cuda()), amax_in=ops.amax_slots(xd))
        torch.cuda.synchronize()
        close(nchw(y), ref, what='cfg %d C%d R%d split %d' % (cfg, C, R, splitk))


def test_f16x2_weight_planes_layout_and_exactness():
    """ppy_conv2d_split_weights_f16x2: planes are chunk-major [2][Kred/32][K][32] (include/ppyolo_hip.h), every channel is
    scaled by its own power of two, hi + lo reproduces w * s to 2^-22 relative, and scale_out = scale / s."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(21)
    K, R, C = 40, 3, 64
    w = (torch.randn(K, R, R, C, generator=g) * torch.exp(2 * torch.randn(K, 1, 1, 1, generator=g))).cuda()
    scale = (torch.rand(K, generator=g) + 0.5).cuda()
    planes, sc = ops.split_weights_f16x2(w, scale)
    kred = R * R * C
    pl = planes.view(torch.float16).view(2, kred // 32, K, 32).permute(0, 2, 1, 3).reshape(2, K, kred).double()
    s_w = (scale.double() / sc.double())                               # the per-channel power of two
    assert torch.equal(torch.log2(s_w), torch.log2(s_w).round()), 'weight scales are not powers of two'
    mx = w.reshape(K, -1).abs().amax(dim=1).double() * s_w
    assert (mx >= 2.0 ** 13).all() and (mx < 2.0 ** 14).all()
    want = w.reshape(K, kred).double() * s_w[:, None]
    err = (pl[0] + pl[1] - want).abs()
    assert (err <= want.abs() * 2.0 ** -22 + 2.0 ** -25).all()
    assert (pl[1].abs() <= pl[0].abs() * 2.0 ** -10 + 2.0 ** -24).all()       # lo is the rounding residual of hi


def test_conv_stride2_upsample_1x1():
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 96, 10, 10, generator=g)
    w = torch.randn(40, 96, 1, 1, generator=g) * 0.1
    one, zero = torch.ones(40), torch.zeros(40)
    ref = F.interpolate(F.relu(F.conv2d(x, w)), scale_factor=2, mode='nearest')
    y = torch.zeros(2, 20, 20, 40).cuda()
    ops.conv2d_bn_act(ops.View(nhwc(x).cuda()), w.permute(0, 2, 3, 1).contiguous().cuda(), one.cuda(), zero.cuda(),
                      ops.View(y), 1, 0, 'relu', upsample2x=True)
    close(nchw(y), ref, what='1x1 + upsample')
    w3 = torch.randn(64, 96, 3, 3, generator=g) * 0.05
    ref = F.conv2d(x, w3, None, 2, 1)
    y = torch.zeros(2, 5, 5, 64).cuda()
    ws = torch.empty(1 << 20).cuda()      # the heuristic may pick split-K for this tiny-M / long-K shape
    ops.conv2d_bn_act(ops.View(nhwc(x).cuda()), w3.permute(0, 2, 3, 1).contiguous().cuda(), torch.ones(64).cuda(),
                      torch.zeros(64).cuda(), ops.View(y), 2, 1, None, ws=ws)
    close(nchw(y), ref, what='3x3 stride 2')


def test_coordconv_as_position_bias(golden):
    """CoordConv + conv (reference custom_layers.py:256-272 then Conv2dUnit) == conv on the
    first C channels + precomputed bias map; checked against the golden CoordConv output."""
    from model.custom_layers import Conv2dUnit
    from ppyolo_hip import engine
    g = golden('g3_coord_spp')
    x, xc = T(g['coord_x']), T(g['coord_y'])
    assert torch.equal(orc.coord_concat(x), xc)
    gen = torch.Generator().manual_seed(3)
    for k in (1, 3):
        u = Conv2dUnit(34, 48, k, stride=1, bn=1, act='leaky')
        with torch.no_grad():
            u.conv.weight.copy_(torch.randn(u.conv.weight.shape, generator=gen) * 0.1)
            u.bn.running_mean.copy_(torch.randn(48, generator=gen) * 0.1)
            u.bn.running_var.copy_(torch.rand(48, generator=gen) + 0.5)
        u.eval()
        sd = {'u.' + n: v for n, v in u.state_dict().items()}
        ref = orc.conv_unit(sd, 'u', xc, 1, 'leaky')
        u = u.cuda()
        b = engine.Builder(x.shape[0], x.shape[2], x.shape[3], torch.device('cuda'))
        xin = b.new_act(x.shape[0], x.shape[2], x.shape[3], 32)
        y = u.emit(b, xin, coord=True)
        ex = engine.HipExecutor(b.plan, 'cuda', use_graph=False)
        ex.bufs[xin.buf].copy_(nhwc(x))
        ex.run()
        close(nchw(ex.view(y).dense()), ref, what='coordconv k=%d' % k)


def test_pools_and_spp(golden):
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 64, 17, 22, generator=g)
    xb = torch.zeros(2, 17, 22, 72).cuda()
    xb[..., 8:] = nhwc(x).cuda()
    y = torch.zeros(2, 9, 11, 64).cuda()
    ops.maxpool3x3s2(ops.View(xb, 8, 64), ops.View(y))
    assert torch.equal(nchw(y).cpu(), F.max_pool2d(x, 3, 2, 1))
    y = torch.zeros(2, 8, 11, 64).cuda()
    ops.avgpool2x2(ops.View(xb, 8, 64), ops.View(y))
    close(nchw(y), F.avg_pool2d(x, 2, 2, 0), rel=1e-6, what='avgpool')
    gd = golden('g3_coord_spp')
    for i in range(3):
        x = T(gd['spp%d_x' % i])
        N, C, H, W = x.shape
        buf = torch.zeros(N, H, W, 4 * C).cuda()
        buf[..., :C] = nhwc(x).cuda()
        v = [ops.View(buf, C * k, C) for k in range(4)]
        ops.spp(v[0], v[1], v[2], v[3])
        assert torch.equal(nchw(buf).cpu(), T(gd['spp%d_y' % i])), 'spp case %d' % i


def test_stem_conv(golden):
    g = golden('g1_conv_units')
    # cases 7 and 8 of the fixture are the 3->32 stride-2 stem (exercised in test_conv_units_golden
    # through Conv2dUnit.forward); here: odd sizes + K = 64 through the op directly
    from ppyolo_hip import ops
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, 3, 21, 34, generator=gen)
    w = torch.randn(64, 3, 3, 3, generator=gen) * 0.2
    sc, sh = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen)
    ref = F.relu(F.conv2d(x, w, None, 2, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    y = torch.zeros(3, 11, 17, 64).cuda()
    ops.stem_conv(x.cuda(), w.cuda(), sc.cuda(), sh.cuda(), ops.View(y), 'relu')
    close(nchw(y), ref, what='stem')


def test_stem_on_the_mfma_matches_fp64_as_well_as_the_fma_chain():
    """Round 4: the stem on the bf16 MFMA (stem_conv_mfma_kernel: 27 -> 32 deep, two k-steps, exact 3-term bf16 split, six
    products) against a float64 convolution, next to the fp32 fma chain of the row kernel: no further from exact than that
    chain (x 1.5 + rounding of the result), incl. odd sizes, partial 2 x 64 tiles, the border taps, a padded pixel stride, an
    image 1000 x larger than its neighbour (no scaling in this scheme), and the tracked per-image maxima."""
    from ppyolo_hip import ops
    gen = torch.Generator().manual_seed(13)
    for (N, H, W, ld) in [(2, 37, 150, 32), (1, 64, 259, 40), (3, 9, 130, 32), (2, 608, 608, 32), (1, 15, 18, 32)]:
        x = torch.randn(N, 3, H, W, generator=gen)
        x[0] *= 1000.0
        w = torch.randn(32, 3, 3, 3, generator=gen) * 0.2
        sc, sh = torch.rand(32, generator=gen) + 0.5, torch.randn(32, generator=gen)
        ref = F.relu(F.conv2d(x.double(), w.double(), None, 2, 1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        err = {}
        for mfma in (False, True):
            y = torch.full((N, Ho, Wo, ld), -3.0).cuda()
            amax = ops.amax_slots(device='cuda', N=N)
            ops.stem_conv(x.cuda(), w.cuda(), sc.cuda(), sh.cuda(), ops.View(y, 0, 32), 'relu', amax_out=amax, mfma=mfma)
            torch.cuda.synchronize()
            out = y.cpu()
            assert bool((out[..., 32:] == -3.0).all()), 'wrote beyond its 32 channels'
            got = out[..., :32].permute(0, 3, 1, 2).double()
            # error per image relative to that image's magnitude (image 0 is 1000 x larger)
            e = [float((got[n] - ref[n]).abs().max() / ref[n].abs().max().clamp_min(1e-30)) for n in range(N)]
            err[mfma] = e
            mx = amax.view(N, -1).amax(dim=1).cpu()
            assert torch.equal(mx, out[..., :32].abs().amax(dim=(1, 2, 3))), 'tracked maxima'
        for n in range(N):
            assert err[True][n] <= 1.5 * err[False][n] + 1.2e-7, ((N, H, W), n, err)
    print('stem: max error / max|y| per image, fma chain %s, bf16x3 MFMA %s' % (['%.1e' % v for v in err[False]], ['%.1e' % v for v in err[True]]))


def test_stem_row_kernel_is_bit_identical_to_the_pixel_kernel():
    """Round 3: the stem as row segments through LDS (csrc/stem_pool.hip, stem_conv_row_kernel) keeps the fma chain of the
    thread-per-pixel form (PPY_STEM_OLD=1 selects it per call): same bits, incl. several / partial 64-pixel segments, odd
    sizes, the image border taps, a padded pixel stride, and the tracked per-image maxima."""
    import os
    from ppyolo_hip import ops
    gen = torch.Generator().manual_seed(11)
    for (N, H, W, K, ld) in [(2, 37, 150, 32, 32), (1, 64, 259, 32, 40), (3, 9, 130, 64, 64), (2, 608, 608, 32, 32)]:
        x = torch.randn(N, 3, H, W, generator=gen).cuda()
        x[0] *= 7.0
        w = (torch.randn(K, 3, 3, 3, generator=gen) * 0.2).cuda()
        sc, sh = (torch.rand(K, generator=gen) + 0.5).cuda(), torch.randn(K, generator=gen).cuda()
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        got = {}
        for form in ('0', '1'):
            os.environ['PPY_STEM_OLD'] = form
            try:
                y = torch.full((N, Ho, Wo, ld), -3.0).cuda()
                amax = ops.amax_slots(device='cuda', N=N)
                ops.stem_conv(x, w, sc, sh, ops.View(y, 0, K), 'relu', amax_out=amax)
                torch.cuda.synchronize()
            finally:
                os.environ.pop('PPY_STEM_OLD', None)
            got[form] = (y.cpu(), amax.view(N, -1).amax(dim=1).cpu())
        assert torch.equal(got['0'][0], got['1'][0]), (N, H, W, K)
        assert torch.equal(got['0'][1], got['1'][1]), 'tracked maxima differ'
        assert torch.equal(got['0'][1], got['0'][0][..., :K].reshape(N, -1).abs().amax(dim=1))
        if ld > K:
            assert bool((got['0'][0][..., K:] == -3.0).all()), 'channels beyond K were written'


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [
    # N, H, W, C, K, stride        (stage-5 shapes of R50vd in small, ragged tiles, K % 4 != 0 = scalar epilogue)
    (2, 19, 19, 64, 128, 1), (3, 13, 11, 96, 72, 2), (1, 9, 9, 32, 33, 1), (2, 20, 20, 128, 256, 2), (8, 19, 19, 64, 64, 1)])
def test_dcn_fused_matches_the_columns_path(shape):
    """The fused DCNv2 kernel (csrc/dcn_fused.hip: gather inside the contraction, no columns buffer) against the columns
    of ppy_dcnv2_sample_f32 -- bit-equal to the reference's gather, test below -- contracted in float64: every math
    scheme x tile x split-K, offsets up to +-12 px (far outside the image), masks on both sigmoid tails."""
    from ppyolo_hip import ops
    N, H, W, C, K, stride = shape
    g = torch.Generator().manual_seed(N * 1000 + C + K)
    Ho, Wo = ops.dcn_out_hw(H, W, stride, 1)
    x = torch.randn(N, H, W, C, generator=g).cuda()
    om = torch.randn(N, Ho, Wo, 27, generator=g)
    om[..., :18] *= 3.0
    om[0, :, :, :18] *= 4.0                     # image 0: most samples land in the padding
    om[..., 18:] *= 4.0
    om = om.cuda()
    w = (torch.randn(K, 3, 3, C, generator=g) * (1.0 / (9 * C)) ** 0.5).cuda()
    scale = (torch.rand(K, generator=g) + 0.5).cuda()
    shift = torch.randn(K, generator=g).cuda()
    M = N * Ho * Wo
    cols = torch.empty(M, 9 * C, device='cuda')
    ops.dcnv2_sample(ops.View(x), ops.View(om), cols, stride, 1)
    ref = cols.double() @ w.reshape(K, -1).double().t() * scale.double() + shift.double()
    ref = torch.where(ref > 0, ref, 0.1 * ref).float().view(N, Ho, Wo, K)
    w3, wf, amax = ops.split_weights_bf16x3(w), ops.split_weights_f16x2(w, scale), ops.amax_slots(x)
    ncfg = ops.dcnv2_num_configs()
    assert ncfg >= 3 * ops.DCN_TILES_4W + 2      # three schemes x six four-wave tiles, then the eight-wave f16x2 tiles
    worst = {}
    for cfg in list(range(ncfg)) + [-1]:
        for splitk in (1, 2, 3, 9) if cfg >= 0 else (0,):
            need = ops.dcnv2_workspace_bytes(N, H, W, C, K, stride, 1, cfg, splitk)
            assert need <= 9 * M * K * 4         # split-K partials only: no N*Ho*Wo*9*C columns
            assert splitk > 1 or cfg < 0 or need == 0
            ws = torch.empty(max(need // 4, 1), device='cuda')
            y = torch.full((N, Ho, Wo, K), float('nan'), device='cuda')
            amax_out = ops.amax_slots(device='cuda', N=N)
            ops.dcnv2(ops.View(x), w, scale, shift, ops.View(om), ops.View(y), stride, 1, 'leaky', ws, cfg=cfg, splitk=splitk,
                      w_x3=w3, w_f16=wf, amax_in=amax, amax_out=amax_out)
            err = float((y - ref).abs().max() / ref.abs().max())
            scheme = 'auto' if cfg < 0 else ops.dcnv2_scheme(cfg)
            worst[scheme] = max(worst.get(scheme, 0.0), err)
            assert err <= 2e-6, (cfg, splitk, err)
            got = amax_out.view(N, -1).amax(dim=1)
            assert torch.allclose(got, y.reshape(N, -1).abs().amax(dim=1), rtol=0, atol=0), (cfg, splitk)
    print('fused DCNv2 %s: max error relative to max|y| per scheme: %s' % (shape, {k: '%.1e' % v for k, v in worst.items()}))
    # schemes without their operands are refused, not silently replaced
    with pytest.raises(Exception):
        ops.dcnv2(ops.View(x), w, scale, shift, ops.View(om), ops.View(y), stride, 1, None, ws, cfg=ncfg - 1, splitk=1)


def test_dcn_gather_and_full_layer(golden):
    from model.custom_layers import Conv2dUnit
    from ppyolo_hip import ops
    g = golden('g2_dcnv2')
    for i in range(int(g['ncases'])):
        p = 'd%d_' % i
        ci, co, s = [int(v) for v in g[p + 'meta']]
        x, om = T(g[p + 'x']), T(g[p + 'offset_mask'])
        N, _, H, W = x.shape
        Ho, Wo = om.shape[2], om.shape[3]
        # (a) the gather alone, from the reference's own offsets: op-for-op arithmetic
        cols = torch.zeros(N * Ho * Wo, 9 * ci).cuda()
        ops.dcnv2_sample(ops.View(nhwc(x).cuda()), ops.View(nhwc(om).cuda()), cols, s, 1)
        ref = orc.dcnv2_sample(x, om[:, :18], torch.sigmoid(om[:, 18:]), s, 1, 3).reshape(N * Ho * Wo, 9 * ci)
        close(cols, ref, rel=2e-6, what='dcn gather %d' % i)
        # (b) the whole deformable layer through the reference-compatible module
        u = Conv2dUnit(ci, co, 3, stride=s, use_dcn=True, act=None)
        with torch.no_grad():
            u.conv.conv_offset.weight.copy_(T(g[p + 'w_off']))
            u.conv.conv_offset.bias.copy_(T(g[p + 'b_off']))
            u.conv.dcn_weight.copy_(T(g[p + 'w_dcn']))
        y = u.eval().cuda()(x.cuda())
        # offsets are recomputed on the GPU (fp32 reordering ~1e-6 px) -> samples move ~1e-5
        e = close(y, T(g[p + 'y']), rel=2e-5, what='dcn layer %d' % i)      # measured on MI355X: 2.8e-6 .. 4.8e-6
        print('dcn layer %d: max error / max|y| %.3e' % (i, e))


# ------------------------------------------------------------------------------------------
def _cand_bufs(N, cap):
    return (torch.zeros(N, cap, dtype=torch.int32).cuda(), torch.zeros(N, cap, dtype=torch.int32).cuda(),
            torch.zeros(N, dtype=torch.int32).cuda())


def test_decode_golden(golden):
    from ppyolo_hip import ops
    g = golden('g4_decode')
    anchors, im_size = g['anchors'], T(g['im_size'])
    for i in range(3):
        meta = [int(v) for v in g['l%d_meta' % i]]
        S, stride, iou_aware, mask = meta[0], meta[1], meta[2], meta[3:]
        o = T(g['l%d_out' % i])
        N = o.shape[0]
        M = S * S * 3
        boxes = torch.zeros(N, M, 4).cuda()
        dense = torch.zeros(N, M, 80).cuda()
        ck, ci, cc = _cand_bufs(N, M * 80)
        ops.yolo_decode(ops.View(nhwc(o).cuda()), anchors[mask].tolist(), stride, 80, 1.05, bool(iou_aware), 0.4, True,
                        im_size.cuda(), boxes, 0, 0.01, ck, ci, cc, dense)
        rb, rs = T(g['l%d_boxes' % i]), T(g['l%d_scores' % i])
        assert (boxes.cpu() - rb).abs().max() <= 1e-3, 'boxes lvl %d: %g' % (i, (boxes.cpu() - rb).abs().max())
        assert (dense.cpu() - rs).abs().max() <= 1e-4
        # tighter: relative 1e-5 (exp/pow ulp differences only)
        assert ((boxes.cpu() - rb).abs() <= 1e-5 * rb.abs().clamp(min=1.0)).all()
        assert np.array_equal(np.signbit(boxes.cpu().numpy()), np.signbit(rb.numpy())), '-0.0 of the x0*0 clip'
        # candidate list == {score > thr} of the kernel's own dense scores
        n_ref = (dense > 0.01).flatten(1).sum(1).cpu()
        assert torch.equal(cc.cpu().long(), n_ref)
        for n in range(N):
            k = int(cc[n])
            got = set(ci[n, :k].cpu().tolist())
            want = set(torch.nonzero(dense[n].flatten() > 0.01).flatten().cpu().tolist())
            assert got == want


def _decode_levels(outs, anchors_px, strides, iou_aware, im_size, thr, staged):
    """All levels through ppy_yolo_decode_levels_f32 on padded NHWC rows (pixel stride = channels rounded up to 4, as the plan
    lays the head outputs out); staged=True forces the round-1/2 LDS-staged kernel.  -> boxes, per image sorted (idx, key)."""
    import os
    from ppyolo_hip import ops
    N = outs[0].shape[0]
    views, M = [], 0
    for o in outs:
        nch = o.shape[1]
        ld = (nch + 3) // 4 * 4
        buf = torch.full((N, o.shape[2], o.shape[3], ld), 123.0).cuda()         # (the pad channels must never be read as classes)
        buf[..., :nch] = nhwc(o).cuda()
        views.append(ops.View(buf, 0, nch))
        M += o.shape[2] * o.shape[3] * 3
    boxes = torch.zeros(N, M, 4).cuda()
    ck, ci, cc = _cand_bufs(N, M * 80)
    from ppyolo_hip._lib import lib
    lib().ppy_debug_decode_mode(1 if staged else 0, -1, 0)          # (the library reads its environment switches once per process)
    try:
        ops.yolo_decode_levels(views, anchors_px, strides, 80, 1.05, iou_aware, 0.4, True, im_size.cuda(), boxes, thr, ck, ci, cc)
        torch.cuda.synchronize()
    finally:
        lib().ppy_debug_decode_mode(-1, -1, 0)
    cands = []
    for n in range(N):
        k = int(cc[n])
        pairs = torch.stack([ci[n, :k].long(), ck[n, :k].long() & 0xffffffff], 1).cpu()
        cands.append(pairs[torch.argsort(pairs[:, 0])])
    return boxes.cpu(), cands


@pytest.mark.parametrize('iou_aware', [True, False])
def test_streaming_decode_is_bit_identical_to_the_staged_kernel(iou_aware, golden):
    """The round-3 streaming decode kernel (registers + quad permutes, no LDS copy, no workgroup barrier) against the staged
    kernel on the same inputs: boxes bit for bit, candidate SETS (index, score key) equal -- three levels incl. one whose cell
    count is not a multiple of the 16-cell groups, realistic and all-pass score regimes, batch 8; and against the reference's
    own yolo_box outputs (golden g4) through the padded-row layout."""
    g = torch.Generator().manual_seed(5)
    N, nch = 8, 3 * 85 + (3 if iou_aware else 0)
    anchors = [[[116, 90], [156, 198], [373, 326]], [[30, 61], [62, 45], [59, 119]], [[10, 13], [16, 30], [33, 23]]]
    strides = [32, 16, 8]
    im_size = torch.tensor([[480., 640.], [375., 500.], [608., 608.], [1080., 1920.]] * 2)
    for regime, bias in (('realistic', -4.0), ('every pair passes', 0.0)):
        outs = []
        for S in (19, 38, 76):
            o = torch.randn(N, nch, S, S, generator=g) * 1.5
            o[:, (3 if iou_aware else 0):] += bias * 0.5                       # objectness / class logits
            o[0, :, 0, 0] = float('nan')                                       # a NaN cell: never a candidate
            o[1, :, S - 1, S - 1] = 80.0                                       # saturated logits
            outs.append(o)
        b_new, c_new = _decode_levels(outs, anchors, strides, iou_aware, im_size, 0.01, False)
        b_old, c_old = _decode_levels(outs, anchors, strides, iou_aware, im_size, 0.01, True)
        assert np.array_equal(b_new.numpy().view(np.int32), b_old.numpy().view(np.int32)), regime
        tot = 0
        for n in range(N):
            assert torch.equal(c_new[n], c_old[n]), (regime, n, c_new[n].shape, c_old[n].shape)
            tot += c_new[n].shape[0]
        assert tot > 0
        if regime != 'realistic':
            assert tot > 0.5 * N * 22743 * 80
    if iou_aware:          # the reference's own numbers (g4: one image set per level, all IoU-aware)
        gd = golden('g4_decode')
        for i in range(3):
            meta = [int(v) for v in gd['l%d_meta' % i]]
            if not meta[2]:
                continue
            S, stride, mask = meta[0], meta[1], meta[3:]
            o = T(gd['l%d_out' % i])
            b, c = _decode_levels([o], [gd['anchors'][mask].tolist()], [stride], True, T(gd['im_size']), 0.01, False)
            rb, rs = T(gd['l%d_boxes' % i]), T(gd['l%d_scores' % i])
            assert ((b - rb).abs() <= 1e-5 * rb.abs().clamp(min=1.0)).all()
            assert np.array_equal(np.signbit(b.numpy()), np.signbit(rb.numpy()))
            for n in range(o.shape[0]):
                want = torch.nonzero(rs[n].flatten() > 0.01).flatten()
                got = c[n][:, 0]
                # (scores within 1e-6 of the threshold may fall on either side of it)
                edge = set(torch.nonzero((rs[n].flatten() - 0.01).abs() < 1e-6).flatten().tolist())
                assert set(got.tolist()) ^ set(want.tolist()) <= edge


def test_worst_case_regime_full_batch():
    """SURVEY 8(d)'s second regime at the headline batch: 8 images, head logits as a default-initialised head gives them (N(0, 0.1)),
    so EVERY one of the 1 819 440 (box, class) pairs of an image passes the 0.01 threshold -- the case in which the reference sorts
    1.8 M keys per image (model/matrix_nms.py:120).  The streaming multi-level decode + radix-select Matrix-NMS must give exactly
    what the dense route gives on the same scores (staged per-level decode -> dense [N, M, 80] scores -> ppy_nms_candidates_f32 ->
    Matrix-NMS): same candidate count, same rows, same keep indices; rows sorted, at most keep_top_k."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(3)
    N, nch = 8, 258
    anchors = [[[116, 90], [156, 198], [373, 326]], [[30, 61], [62, 45], [59, 119]], [[10, 13], [16, 30], [33, 23]]]
    strides, sizes = [32, 16, 8], [19, 38, 76]
    im_size = torch.tensor([[480., 640.], [375., 500.], [608., 608.], [1080., 1920.]] * 2).cuda()
    M = sum(S * S * 3 for S in sizes)
    views, dense_views = [], []
    for S in sizes:
        buf = torch.zeros(N, S, S, 260).cuda()
        buf[..., :nch] = (torch.randn(N, S, S, nch, generator=g) * 0.1).cuda()
        views.append(ops.View(buf, 0, nch))
    boxes = torch.zeros(N, M, 4).cuda()
    ck, ci, cc = _cand_bufs(N, M * 80)
    ops.yolo_decode_levels(views, anchors, strides, 80, 1.05, True, 0.4, True, im_size, boxes, 0.01, ck, ci, cc)

    def nms(ck_, ci_, cc_, bx):
        dets = torch.zeros(N, 100, 6).cuda()
        cnt = torch.zeros(N, dtype=torch.int32).cuda()
        keep = torch.zeros(N, 100, dtype=torch.int32).cuda()
        ops.matrix_nms(bx, 80, ck_, ci_, cc_, 0.01, 500, 100, False, 2.0, dets, cnt, keep)
        torch.cuda.synchronize()
        return dets.cpu(), cnt.cpu(), keep.cpu()
    d1, n1, k1 = nms(ck, ci, cc, boxes)
    assert torch.equal(cc.cpu(), torch.full((N,), M * 80, dtype=torch.int32)), 'every pair is a candidate'
    # the dense route on the same head outputs
    boxes2 = torch.zeros(N, M, 4).cuda()
    dense = torch.zeros(N, M, 80).cuda()
    ck2, ci2, cc2 = _cand_bufs(N, M * 80)
    off = 0
    for v, a, st, S in zip(views, anchors, strides, sizes):
        ops.yolo_decode(v, a, st, 80, 1.05, True, 0.4, True, im_size, boxes2, off, 0.01, ck2, ci2, cc2, dense)
        off += S * S * 3
    assert np.array_equal(boxes.cpu().numpy().view(np.int32), boxes2.cpu().numpy().view(np.int32))
    ck3, ci3, cc3 = _cand_bufs(N, M * 80)
    ops.nms_candidates(dense, 0.01, ck3, ci3, cc3)
    d2, n2, k2 = nms(ck3, ci3, cc3, boxes2)
    assert torch.equal(n1, n2) and torch.equal(d1, d2) and torch.equal(k1, k2)
    for n in range(N):
        k = int(n1[n])
        assert 1 <= k <= 100 and torch.all(d1[n, :k - 1, 1] >= d1[n, 1:k, 1])
        # the best pair of the image is kept first, undecayed
        assert float(d1[n, 0, 1]) == float(dense[n].max())


def _run_nms(boxes, scores, cfg):
    from ppyolo_hip import ops
    N, M, C = scores.shape
    thr, post, topk, keepk, gauss, sigma = cfg
    ck, ci, cc = _cand_bufs(N, M * C)
    ops.nms_candidates(scores.cuda(), thr, ck, ci, cc)
    dets = torch.zeros(N, keepk, 6).cuda()
    cnt = torch.zeros(N, dtype=torch.int32).cuda()
    keep = torch.zeros(N, keepk, dtype=torch.int32).cuda()
    ops.matrix_nms(boxes.cuda(), C, ck, ci, cc, post, topk, keepk, gauss, sigma, dets, cnt, keep)
    torch.cuda.synchronize()
    return dets.cpu(), cnt.cpu(), keep.cpu()


def test_matrix_nms_golden_bit_exact(golden):
    g = golden('g5_matrix_nms')
    for i in range(int(g['ncases'])):
        c = g['n%d_cfg' % i]
        cfg = (float(np.float32(c[0])), float(np.float32(c[1])), int(c[2]), int(c[3]), bool(c[4]), float(c[5]))
        b, s, ref = T(g['n%d_boxes' % i]), T(g['n%d_scores' % i]), T(g['n%d_pred' % i])
        dets, cnt, keep = _run_nms(b[None], s[None], cfg)
        k = int(cnt[0])
        if ref[0, 0] < 0:
            assert k == 0, 'case %d: expected the empty sentinel' % i
            assert torch.all(dets == -1)
            continue
        assert k == ref.shape[0], 'case %d: %d rows vs %d' % (i, k, ref.shape[0])
        got = dets[0, :k]
        assert torch.equal(got[:, 0], ref[:, 0]), 'case %d labels' % i
        assert torch.equal(got[:, 2:], ref[:, 2:]), 'case %d boxes' % i
        if cfg[4]:      # gaussian kernel uses exp(): ulp-level differences allowed
            assert (got[:, 1] - ref[:, 1]).abs().max() <= 1e-6
        else:
            assert torch.equal(got[:, 1], ref[:, 1]), 'case %d scores not bit-exact' % i
        # keep indices: the oracle's flat candidate index of every kept row
        _, f = orc.matrix_nms(b, s, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], return_index=True)
        assert np.array_equal(keep[0, :k].numpy().astype(np.int64), f), 'case %d keep indices' % i
        assert torch.all(keep[0, k:] == -1) and torch.all(dets[0, k:] == -1)


def test_matrix_nms_full_size_every_pair_a_candidate():
    """BASELINE-sized stress: 22743 boxes x 80 classes, EVERY pair above the threshold
    (1.8 M candidates per image; the reference sorts them all) -> radix-select path."""
    g = torch.Generator().manual_seed(21)
    M, C, N = 22743, 80, 2
    base = torch.rand(300, 4, generator=g)
    cx, cy = base[:, 0] * 640, base[:, 1] * 480
    bw, bh = base[:, 2] * 150 + 10, base[:, 3] * 150 + 10
    base = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    boxes = base[torch.randint(0, 300, (N, M), generator=g)] + torch.randn(N, M, 4, generator=g) * 4
    scores = torch.empty(N, M * C)
    for n in range(N):
        scores[n] = (torch.randperm(M * C, generator=g).float() + 1.0) / (M * C + 2) * 0.9 + 0.05   # distinct
    scores = scores.reshape(N, M, C)
    dets, cnt, keep = _run_nms(boxes, scores, (0.01, 0.01, 500, 100, False, 2.0))
    for n in range(N):
        ref, f = orc.matrix_nms(boxes[n], scores[n], 0.01, 0.01, 500, 100, False, 2.0, return_index=True)
        k = int(cnt[n])
        assert k == ref.shape[0]
        assert torch.equal(dets[n, :k], ref)
        assert np.array_equal(keep[n, :k].numpy().astype(np.int64), f)


def _nms_big_header(ws, N):
    """(ccount, bad) per image of the large-list header behind the NmsWs array (csrc/decode_nms.hip: NmsBig)."""
    from ppyolo_hip._lib import lib
    one = int(lib().ppy_matrix_nms_workspace_bytes(1))
    per_ws = one - 64 - 2 * 32768 * 4
    raw = ws.view(torch.int32).cpu()
    hdr = raw[N * per_ws // 4:N * per_ws // 4 + 16 * N].view(N, 16)
    return hdr[:, 1].tolist(), hdr[:, 2].tolist()


@pytest.mark.parametrize('case', ['mid', 'mixed', 'ties', 'few_above'])
def test_matrix_nms_large_lists_take_the_compact_route(case):
    """Round 4: a candidate list that does not fit the select kernel's LDS cache (> 8192 entries) is cut down chip-wide first
    (nms_sample_kernel -> a score threshold from 8192 sampled keys; nms_collect_kernel -> every entry at or above it, counted
    exactly) and the select runs on that compact list iff it must contain the whole top-k.  Rows and keep indices equal the
    oracle's on: a mid-size list, a batch mixing small / large / empty lists, massive exact ties (the compact list overflows ->
    the original list is walked as before), and a list whose scores above the sampled threshold are fewer than nms_top_k."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(77)
    C = 80
    cfg = (0.05, 0.01, 500, 100, False, 2.0)

    def boxes_of(M):
        b = torch.rand(M, 4, generator=g) * 500
        b[:, 2:] = b[:, :2] + 5 + torch.rand(M, 2, generator=g) * 120
        return b
    if case == 'mid':            # 3 images x ~20 k / 100 k / 9 k candidates, distinct scores
        Ms, fracs = [1500, 1500, 1500], [0.17, 0.85, 0.076]
    elif case == 'mixed':        # small (LDS-cached), large, empty
        Ms, fracs = [1500, 1500, 1500], [0.02, 0.9, 0.0]
    elif case == 'ties':
        Ms, fracs = [1500, 1500], [0.9, 0.9]
    else:
        Ms, fracs = [1500], [0.9]
    N, M = len(Ms), Ms[0]
    boxes = torch.stack([boxes_of(M) for _ in range(N)])
    scores = torch.zeros(N, M * C)
    for n in range(N):
        k = int(M * C * fracs[n])
        if case == 'ties':       # 15 distinct values: every sampled threshold ties with thousands of entries
            vals = torch.randint(1, 16, (k,), generator=g).float() / 20.0 + 0.1
        elif case == 'few_above':  # 300 scores near 0.9, everything else exactly 0.06: fewer than top_k above any useful threshold
            vals = torch.full((k,), 0.06)
            vals[:300] = 0.9 + torch.randperm(300, generator=g).float() * 1e-4
        else:
            vals = (torch.randperm(k, generator=g).float() + 1.0) / (k + 2) * 0.9 + 0.06
        scores[n, torch.randperm(M * C, generator=g)[:k]] = vals
    scores = scores.reshape(N, M, C)
    ck, ci, cc = _cand_bufs(N, M * C)
    ops.nms_candidates(scores.cuda(), cfg[0], ck, ci, cc)
    dets = torch.zeros(N, 100, 6).cuda()
    cnt = torch.zeros(N, dtype=torch.int32).cuda()
    keep = torch.zeros(N, 100, dtype=torch.int32).cuda()
    ws = ops.matrix_nms_workspace(N, 'cuda')
    ops.matrix_nms(boxes.cuda(), C, ck, ci, cc, cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], dets, cnt, keep, ws=ws)
    torch.cuda.synchronize()
    ccount, bad = _nms_big_header(ws, N)
    counts = cc.cpu().tolist()
    for n in range(N):
        ref, f = orc.matrix_nms(boxes[n], scores[n], *cfg, return_index=True)
        k = int(cnt[n])
        if ref[0, 0] < 0:
            assert k == 0
            continue
        assert k == ref.shape[0], (case, n)
        assert torch.equal(dets[n, :k].cpu(), ref), (case, n)
        assert np.array_equal(keep[n, :k].cpu().numpy().astype(np.int64), f), (case, n)
        if counts[n] <= 8192:
            assert ccount[n] == -1, 'a small list must not be touched'
        elif case in ('mid', 'mixed'):
            assert bad[n] == 0 and 500 <= ccount[n] <= 8192, 'compact route not taken: %d of %d entries' % (ccount[n], counts[n])
        elif case == 'ties':       # the threshold is one of 15 values: thousands of entries tie with it, all of them collected
            assert ccount[n] >= 0.9 * 1500 * 80 / 15 * 0.8
    if case == 'few_above':
        assert ccount[0] >= 500      # the threshold falls into the tie: all of it is counted, the list overflows or is complete


def test_matrix_nms_ties_use_index_order():
    """Exact score ties (the reference's argsort is unstable there): this build's documented
    total order (score desc, candidate index asc) == the oracle's."""
    g = torch.Generator().manual_seed(9)
    M, C = 700, 3
    boxes = torch.rand(M, 4, generator=g) * 300
    boxes[:, 2:] += boxes[:, :2] + 5
    scores = (torch.randint(1, 40, (M, C), generator=g).float() / 64.0)     # many exact ties
    dets, cnt, keep = _run_nms(boxes[None], scores[None], (0.05, 0.01, 500, 100, False, 2.0))
    ref, f = orc.matrix_nms(boxes, scores, 0.05, 0.01, 500, 100, False, 2.0, return_index=True)
    k = int(cnt[0])
    assert k == ref.shape[0]
    assert torch.equal(dets[0, :k], ref)
    assert np.array_equal(keep[0, :k].numpy().astype(np.int64), f)


def test_conv_random_shapes_all_kernels():
    """Seeded sweep over layer shapes x tile configurations x split-K (edge cases: M smaller than a
    tile, K not a multiple of 4 -> scalar epilogue, stride 2 with odd sizes, single-chunk
    reductions, split > chunks) against F.conv2d."""
    import random
    from ppyolo_hip import ops
    from ppyolo_hip._lib import lib
    rnd = random.Random(1234)
    ncfg = lib().ppy_conv2d_num_configs()
    g = torch.Generator().manual_seed(99)
    ws = torch.empty(8 << 20).cuda()
    for case in range(120):
        N = rnd.choice([1, 2, 3])
        C = rnd.choice([32, 64, 96, 160])
        K = rnd.choice([5, 27, 32, 64, 100, 258, 300])
        R = rnd.choice([1, 3])
        stride = rnd.choice([1, 1, 2])
        H, W = rnd.randint(3, 33), rnd.randint(3, 33)
        cfg = rnd.randrange(ncfg)
        splitk = rnd.choice([1, 1, 2, 5, 64])
        act = rnd.choice([None, 'relu', 'leaky'])
        pad = (R - 1) // 2
        x = torch.randn(N, C, H, W, generator=g)
        w = torch.randn(K, C, R, R, generator=g) * (1.0 / (C * R * R) ** 0.5)
        sc, sh = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
        ref = F.conv2d(x, w, None, stride, pad) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        use_res = rnd.random() < 0.5
        res = torch.randn(ref.shape, generator=g) if use_res else None
        if use_res:
            ref = ref + res
        ref = F.relu(ref) if act == 'relu' else (F.leaky_relu(ref, 0.1) if act == 'leaky' else ref)
        Ho, Wo = ref.shape[2], ref.shape[3]
        y = torch.full((N, Ho, Wo, K), 123.0).cuda()
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        def run():
            ops.conv2d_bn_act(ops.View(xd), wk, sc.cuda(), sh.cuda(),
                              ops.View(y), stride, pad, act, residual=None if res is None else ops.View(nhwc(res).cuda()),
                              cfg=cfg, splitk=splitk, ws=ws, w_x3=ops.split_weights_bf16x3(wk),
                              w_f16=ops.split_weights_f16x2(wk, sc.cuda()), amax_in=ops.amax_slots(xd))
        special_ok = True
        fam = ops.conv_cfg(cfg).family
        if fam == 'patch':                # patch kernel: 3x3 / stride 1, C = 32, K = 32 / 64, no shortcut
            special_ok = R == 3 and stride == 1 and C == 32 and K in (32, 64) and not use_res and splitk == 1
        elif fam == 'stream':          # streaming kernel: 1x1 / stride 1, C = 64 / 128, whole channel slices
            special_ok = R == 1 and stride == 1 and splitk == 1 and H * W >= 32 and ((C == 64 and K in (32 * 2, 128, 256)) or (C == 128 and K in (128, 256)))
        if (fam == 'f16x2_slab' and not (R == 3 and stride == 1)) or not special_ok:        # refused loudly, no silent other kernel
            from ppyolo_hip._lib import PPYoloHipError
            with pytest.raises(PPYoloHipError):
                run()
            continue
        run()
        torch.cuda.synchronize()
        close(nchw(y), ref, what='case %d: N%d C%d K%d R%d s%d %dx%d cfg%d split%d' % (case, N, C, K, R, stride, H, W, cfg,
                                                                                 splitk))


def test_bf16x3_split_is_exact_and_fp32_grade():
    """The three bf16 planes of the weights sum back to the fp32 value exactly, the bf16x3 kernel needs them
    (BAD_ARG without), and against an fp64 reference its error is at the level of the exact-fp32 MFMA kernel."""
    from ppyolo_hip import ops
    from ppyolo_hip._lib import PPYoloHipError
    g = torch.Generator().manual_seed(5)
    N, H, W, C, K = 2, 24, 24, 256, 128
    x = torch.randn(N, C, H, W, generator=g).abs() * torch.exp(2 * torch.randn(N, C, H, W, generator=g))
    w = torch.randn(K, C, 3, 3, generator=g) * 0.03
    wk = w.permute(0, 2, 3, 1).contiguous().cuda()
    planes = ops.split_weights_bf16x3(wk)
    as_f32 = (planes.to(torch.int32) << 16).view(torch.float32)            # bf16 bits -> fp32 value
    assert torch.equal((as_f32[0] + as_f32[1]) + as_f32[2], wk), 'split is not exact'
    assert (as_f32[1].abs() <= as_f32[0].abs() * 2.0 ** -8 + 1e-45).all()
    one, zero = torch.ones(K).cuda(), torch.zeros(K).cuda()
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)
    errs = {}
    xd = nhwc(x).cuda()
    wf = ops.split_weights_f16x2(wk, one)
    for name, cfg, wx in (('fp32', 19, None), ('bf16x3', 31, planes), ('bf16x3-b', 32, planes), ('f16x2', 40, None),
                          ('f16x2-b', 44, None)):
        y = torch.zeros(N, H, W, K).cuda()
        ops.conv2d_bn_act(ops.View(xd), wk, one, zero, ops.View(y), 1, 1, None, cfg=cfg, splitk=1, w_x3=wx,
                          w_f16=wf if cfg >= 40 else None, amax_in=ops.amax_slots(xd) if cfg >= 40 else None)
        torch.cuda.synchronize()
        errs[name] = (((nchw(y).cpu().double() - ref) / mag) ** 2).mean().sqrt().item()
    print('rms error / sum|a*b| vs fp64:', errs)
    assert all(errs[k] <= 1.25 * errs['fp32'] for k in errs), errs
    with pytest.raises(PPYoloHipError):
        ops.conv2d_bn_act(ops.View(nhwc(x).cuda()), wk, one, zero, ops.View(y), 1, 1, None, cfg=31, splitk=1)


@pytest.mark.parametrize('case', ['zeros', 'tiny', 'huge', 'outlier', 'negative_only', 'loose_bound'])
def test_f16x2_extreme_ranges(case):
    """The f16x2 kernels scale their input by a power of two derived from the tracked tensor maximum: all-zero,
    1e-6-sized, 1e6-sized and outlier-dominated tensors, and a maximum that is only a loose upper bound (as for pooled
    tensors), must all stay at the fp32 kernel's error level against an fp64 reference."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(11)
    N, H, W, C, K = 1, 20, 20, 128, 96
    x = torch.randn(N, C, H, W, generator=g).abs() * torch.exp(2 * torch.randn(N, C, H, W, generator=g))
    amax_mul = 1.0
    if case == 'zeros':
        x = torch.zeros_like(x)
    elif case == 'tiny':
        x = x * 1e-6
    elif case == 'huge':
        x = x * 1e6
    elif case == 'outlier':
        x[0, 3, 5, 7] = 3e4
    elif case == 'negative_only':
        x = -x
    elif case == 'loose_bound':
        amax_mul = 37.0
    w = torch.randn(K, C, 3, 3, generator=g) * 0.03
    w[5] *= 1e-5                 # output channels with very different weight magnitudes get their own scale
    w[6] *= 1e4
    w[7] = 0.0
    wk = w.permute(0, 2, 3, 1).contiguous().cuda()
    xd = nhwc(x).cuda()
    one, zero = torch.ones(K).cuda(), torch.zeros(K).cuda()
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1) + 1e-300
    errs = {}
    for name, cfg in (('fp32', 19), ('f16x2', 44), ('f16x2-b', 41)):
        y = torch.full((N, H, W, K), 7.0).cuda()
        ops.conv2d_bn_act(ops.View(xd), wk, one, zero, ops.View(y), 1, 1, None, cfg=cfg, splitk=1,
                          w_f16=ops.split_weights_f16x2(wk, one), amax_in=ops.amax_slots(xd) * amax_mul)
        torch.cuda.synchronize()
        got = nchw(y).cpu().double()
        assert torch.isfinite(got).all(), (case, name)
        errs[name] = (((got - ref) / mag) ** 2).mean().sqrt().item()
        if case == 'zeros':
            assert (got == 0).all()
        assert (got[:, 7] == 0).all(), 'all-zero weight row'
    print(case, errs)
    if case != 'zeros':
        assert errs['f16x2'] <= 1.5 * errs['fp32'] + 1e-9 and errs['f16x2-b'] <= 1.5 * errs['fp32'] + 1e-9, (case, errs)


def test_f16x2_images_are_independent():
    """Per-image activation scales: the result for an image is bit-identical whether it runs alone or in a batch whose
    other image is 1e4 times larger (tracked maxima produced by a preceding conv launch, as in the model)."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(3)
    H, W, C, K = 18, 14, 64, 128
    x0 = torch.randn(1, C, H, W, generator=g)
    x1 = torch.randn(1, C, H, W, generator=g) * 1e4
    w1 = torch.randn(C, C, 1, 1, generator=g) * 0.1
    w2 = torch.randn(K, C, 3, 3, generator=g) * 0.05
    one, zero = torch.ones(C).cuda(), torch.zeros(C).cuda()
    onek, zerok = torch.ones(K).cuda(), torch.zeros(K).cuda()

    def run(x):
        N = x.shape[0]
        xd = nhwc(x).cuda()
        w1k, w2k = w1.permute(0, 2, 3, 1).contiguous().cuda(), w2.permute(0, 2, 3, 1).contiguous().cuda()
        mid, out = torch.zeros(N, H, W, C).cuda(), torch.zeros(N, H, W, K).cuda()
        am = ops.amax_slots(device='cuda', N=N)
        ops.conv2d_bn_act(ops.View(xd), w1k, one, zero, ops.View(mid), 1, 0, 'relu', cfg=15, amax_out=am)      # producer
        ops.conv2d_bn_act(ops.View(mid), w2k, onek, zerok, ops.View(out), 1, 1, None, cfg=44, splitk=1,
                          w_f16=ops.split_weights_f16x2(w2k, onek), amax_in=am)                                 # f16x2 consumer
        torch.cuda.synchronize()
        return out.cpu(), am.view(N, -1).amax(dim=1).cpu(), mid.cpu()

    alone, am_alone, _ = run(x0)
    both, am_both, mid = run(torch.cat([x0, x1]))
    assert torch.equal(am_both, mid.reshape(2, -1).abs().amax(dim=1)) and am_both[0] == am_alone[0]
    assert torch.equal(both[0], alone[0]), 'image 0 depends on the other image of the batch'
    ref = F.conv2d(F.relu(F.conv2d(x1.double(), w1.double())), w2.double(), None, 1, 1)
    assert ((nchw(both[1:]).double() - ref).abs().max() / ref.abs().max()) < 1e-5


@pytest.mark.parametrize('case', ['constant', 'low_bits_set', 'same_sign_residuals', 'cancelling', 'wide_range'])
def test_f16x2_adversarial_max_error(case):
    """Worst-case (not rms) error of the f16x2 scheme on the longest reduction of the model (K = 9*512 = 4608) with
    operands built so that the representation errors of the 2-term fp16 split do NOT average out: identical values,
    every dropped mantissa bit set, residuals of one sign, exact cancellation, and activations spread over 2^20 within one
    image.  Compared by MAXIMUM error relative to sum|a*b| against float64, next to the exact-fp32 MFMA kernel on the same
    data (a k-ordered fma chain with one rounding per product).  Analytic bound of the split itself: |a*s - a0 - a1| <=
    2^-24 |a*s| per operand plus the dropped a1*b1 <= 2^-24 |ab|, i.e. <= 3 * 2^-24 = 1.8e-7 of sum|ab| even when every
    error has the same sign; the accumulation (one fp32 rounding per 16 products instead of per product) adds less than
    the fp32 chain's own."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(23)
    N, H, W, C, K = 1, 16, 16, 512, 64
    if case == 'constant':
        x = torch.full((N, C, H, W), 1.9999999)             # 0x3FFFFFFF: every mantissa bit set
        w = torch.full((K, C, 3, 3), 0.33333334)
    elif case == 'low_bits_set':
        x = (torch.randn(N, C, H, W, generator=g).abs() + 0.5).view(torch.int32).bitwise_or(0x1FFF).view(torch.float32)
        w = (torch.randn(K, C, 3, 3, generator=g) * 0.05).view(torch.int32).bitwise_or(0x1FFF).view(torch.float32)
    elif case == 'same_sign_residuals':
        # values just above an fp16 grid point of the scaled operand: the first residual is always +, never rounds to even
        x = (torch.randint(1024, 2048, (N, C, H, W), generator=g).float() + 0.2499) / 128.0
        w = (torch.randint(1024, 2048, (K, C, 3, 3), generator=g).float() + 0.2499) / 65536.0
    elif case == 'cancelling':
        x = torch.full((N, C, H, W), 1.2345678)
        w = torch.full((K, C, 3, 3), 0.7654321)
        w[:, 1::2] *= -1.0                                  # the exact sum is 0 at interior pixels
    else:
        x = torch.exp2(-20.0 * torch.rand(N, C, H, W, generator=g)) * 1000.0
        w = torch.randn(K, C, 3, 3, generator=g) * 0.05
    wk = w.permute(0, 2, 3, 1).contiguous().cuda()
    xd = nhwc(x).cuda()
    one, zero = torch.ones(K).cuda(), torch.zeros(K).cuda()
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)
    errs = {}
    for name, cfg in (('fp32', 19), ('f16x2 128x64', 44), ('f16x2 128x128', 41), ('f16x2 256x128 3 stages', 49),
                      ('f16x2 64x64 4 stages', 66)):
        y = torch.full((N, H, W, K), 7.0).cuda()
        ops.conv2d_bn_act(ops.View(xd), wk, one, zero, ops.View(y), 1, 1, None, cfg=cfg, splitk=1,
                          w_f16=ops.split_weights_f16x2(wk, one), amax_in=ops.amax_slots(xd))
        torch.cuda.synchronize()
        errs[name] = ((nchw(y).cpu().double() - ref).abs() / mag).max().item()
    print(case, {k: '%.3e' % v for k, v in errs.items()})
    for k, v in errs.items():
        if k != 'fp32':
            assert v <= max(1.5 * errs['fp32'], 3 * 2.0 ** -24), (case, errs)


@pytest.mark.parametrize('cfg', range(SLAB0, SLAB1))
def test_slab_reuse_edge_shapes(cfg):
    """The slab variants of the f16x2 kernels (one BM+8-row slab per (channel chunk, r) serves the taps s = 0..2): maps one
    pixel wide / high, tiles that straddle several images, M far below a tile, one chunk of channels (9 chunks, splits that
    do not divide them), reductions shorter than the stage count, and padding taps zeroed through the activation scale --
    against F.conv2d; plus bit-identity with the plain f16x2 kernel of the same tile (same products, same order)."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(900 + cfg)
    ws = torch.empty(4 << 20).cuda()
    for N, H, W, C, K, splitk in ((1, 1, 1, 32, 40, 1), (3, 1, 7, 64, 72, 2), (2, 9, 1, 32, 100, 1), (5, 2, 2, 96, 64, 4),
                                  (2, 19, 19, 64, 136, 1), (1, 33, 31, 32, 258, 2), (4, 6, 5, 160, 48, 5), (2, 13, 11, 32, 64, 9)):
        x = torch.randn(N, C, H, W, generator=g) * torch.exp(torch.randn(N, 1, 1, 1, generator=g))
        w = torch.randn(K, C, 3, 3, generator=g) * (1.0 / (9 * C) ** 0.5)
        sc, sh = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
        ref = F.leaky_relu(F.conv2d(x, w, None, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), 0.1)
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        wf = ops.split_weights_f16x2(wk, sc.cuda())
        outs = []
        for c in (cfg, cfg - 27):                       # the slab variant and the plain f16x2 kernel of the same tile / stage count
            y = torch.full((N, H, W, K), 9.0).cuda()
            ops.conv2d_bn_act(ops.View(xd), wk, sc.cuda(), sh.cuda(), ops.View(y), 1, 1, 'leaky', cfg=c, splitk=splitk, ws=ws,
                              w_f16=wf, amax_in=ops.amax_slots(xd))
            torch.cuda.synchronize()
            outs.append(y)
        close(nchw(outs[0]), ref, what='slab cfg %d: N%d %dx%d C%d K%d split %d' % (cfg, N, H, W, C, K, splitk))
        if splitk == 1:
            assert torch.equal(outs[0], outs[1]), 'slab cfg %d differs from the plain kernel (N%d %dx%d C%d K%d)' % (cfg, N, H, W, C, K)


def _amax_per_image(a, N):
    return a.view(N, -1).amax(dim=1)


@pytest.mark.parametrize('variant', (0, 1))
def test_stream_1x1_is_bit_identical_to_the_f16x2_tiles(variant):
    """csrc/conv_stream.hip (persistent streaming kernel for the C = 64 1x1 layers) against the 128x128 f16x2 tile of
    conv_x3.hip: same products in the same order, so y must be EQUAL (and the tracked per-image maxima exact) -- maps whose pixel
    count is no multiple of 32, tiles that straddle images, one / two / four / eight channel slices, with and without the
    shortcut, all activations, outputs that are slices of a wider buffer."""
    from ppyolo_hip import ops
    from ppyolo_hip._lib import lib
    first = ops.stream_first_cfg()
    g = torch.Generator().manual_seed(4100 + variant)
    for C, N, H, W, K, res, act, y_extra in ((64, 2, 24, 20, 256, True, 'relu', 0), (64, 3, 9, 7, 256, True, 'relu', 0), (64, 1, 6, 6, 64, False, None, 0),
                                             (64, 5, 8, 5, 128, True, 'leaky', 64), (64, 2, 40, 40, 512, False, 'relu', 0), (64, 8, 7, 5, 256, True, None, 32),
                                             # C = 128: the tile's activations staged through the LDS, K / 128 workgroups per pixel stream
                                             (128, 2, 24, 20, 512, True, 'relu', 0), (128, 3, 9, 7, 128, False, 'leaky', 0), (128, 5, 8, 5, 256, True, None, 64),
                                             (128, 2, 40, 40, 1024, True, 'relu', 0), (128, 8, 7, 5, 512, True, 'relu', 32)):
        x = torch.randn(N, C, H, W, generator=g) * torch.exp(torch.randn(N, 1, 1, 1, generator=g))
        w = torch.randn(K, C, 1, 1, generator=g) * 0.125
        sc, sh = (torch.rand(K, generator=g) + 0.5).cuda(), torch.randn(K, generator=g).cuda()
        r = (torch.randn(N, H, W, K, generator=g) * 2).cuda() if res else None
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        wf = ops.split_weights_f16x2(wk, sc)
        outs, maxima = [], []
        for c in (first + variant, 41):
            y = torch.full((N, H, W, K + y_extra), 9.0).cuda()
            am = ops.amax_slots(N=N, device=y.device)
            ops.conv2d_bn_act(ops.View(xd), wk, sc, sh, ops.View(y, 0, K), 1, 0, act, residual=None if r is None else ops.View(r),
                              cfg=c, splitk=1, w_f16=wf, amax_in=ops.amax_slots(xd), amax_out=am)
            torch.cuda.synchronize()
            outs.append(y)
            maxima.append(_amax_per_image(am, N))
        what = 'C%d N%d %dx%d K%d res %s act %s' % (C, N, H, W, K, res, act)
        ref = F.conv2d(x, w) * sc.cpu().view(1, -1, 1, 1) + sh.cpu().view(1, -1, 1, 1)
        if res:
            ref = ref + nchw(r.cpu())
        ref = {'relu': F.relu, 'leaky': lambda t: F.leaky_relu(t, 0.1), None: lambda t: t}[act](ref)
        close(nchw(outs[0][..., :K]), ref, what=what)
        assert torch.equal(outs[0], outs[1]), what                      # (including the untouched columns of a wider buffer)
        exact = outs[0][..., :K].reshape(N, -1).abs().amax(dim=1)
        assert torch.equal(maxima[0], exact), what           # (32-row tiles touch at most two images: exact per image)
        assert bool((maxima[1] >= exact).all()), what        # (a 128-row tile over more than two images records an upper bound)


def test_stream_1x1_writes_the_2x2_average_of_its_output():
    """ppy_conv1x1_expand_f32 with `pooled`: y equals the plain f16x2 tile's, pooled equals ppy_avgpool2x2_f32 of it (same
    order of additions) -- blocks of 2x2 pixels as tile rows, images of 9 / 15 / 400 blocks (tiles that straddle images,
    a last tile with fewer than eight blocks), pooled as a slice of a wider buffer."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(4200)
    for C, N, H, W, K, res, variant in ((64, 2, 6, 6, 256, True, 0), (64, 3, 6, 10, 128, True, 1), (64, 2, 40, 40, 256, True, 0), (64, 5, 8, 6, 64, False, 0),
                                        (128, 2, 6, 6, 512, True, 0), (128, 3, 6, 10, 128, True, 1), (128, 2, 40, 40, 512, True, 0), (128, 5, 8, 6, 256, False, 1)):
        x = torch.randn(N, C, H, W, generator=g) * torch.exp(torch.randn(N, 1, 1, 1, generator=g))
        w = torch.randn(K, C, 1, 1, generator=g) * 0.125
        sc, sh = (torch.rand(K, generator=g) + 0.5).cuda(), torch.randn(K, generator=g).cuda()
        r = (torch.randn(N, H, W, K, generator=g) * 2).cuda() if res else None
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        wf = ops.split_weights_f16x2(wk, sc)
        y0 = torch.full((N, H, W, K), 9.0).cuda()
        am0 = ops.amax_slots(N=N, device=y0.device)
        ops.conv2d_bn_act(ops.View(xd), wk, sc, sh, ops.View(y0), 1, 0, 'relu', residual=None if r is None else ops.View(r),
                          cfg=41, splitk=1, w_f16=wf, amax_in=ops.amax_slots(xd), amax_out=am0)
        p0 = torch.zeros(N, H // 2, W // 2, K).cuda()
        ops.avgpool2x2(ops.View(y0), ops.View(p0))
        y1 = torch.full((N, H, W, K), 9.0).cuda()
        p1 = torch.full((N, H // 2, W // 2, K + 32), 5.0).cuda()
        am1 = ops.amax_slots(N=N, device=y0.device)
        ops.conv1x1_expand(ops.View(xd), wf, sh, ops.View(y1), 'relu', None if r is None else ops.View(r), ops.View(p1, 0, K), variant,
                           ops.amax_slots(xd), am1)
        torch.cuda.synchronize()
        what = 'C%d N%d %dx%d K%d' % (C, N, H, W, K)
        assert torch.equal(y0, y1), what
        assert torch.equal(p0, p1[..., :K]), what
        assert bool((p1[..., K:] == 5.0).all()), what
        assert torch.equal(_amax_per_image(am1, N), y1.reshape(N, -1).abs().amax(dim=1)), what


def test_stream_1x1_refuses_what_it_cannot_run():
    """An explicit streaming id on another geometry is an error (PPY_ERR_BAD_ARG), not a silent other kernel."""
    from ppyolo_hip import ops
    from ppyolo_hip._lib import lib, PPYoloHipError
    first = ops.stream_first_cfg()
    for C, K, R in ((256, 256, 1), (64, 96, 1), (64, 64, 3), (128, 192, 1), (128, 384, 1)):
        x = torch.randn(1, 8, 8, C).cuda()
        wk = torch.randn(K, R, R, C).cuda()
        one, zero = torch.ones(K).cuda(), torch.zeros(K).cuda()
        y = torch.zeros(1, 8, 8, K).cuda()
        with pytest.raises(PPYoloHipError):
            ops.conv2d_bn_act(ops.View(x), wk, one, zero, ops.View(y), 1, (R - 1) // 2, None, cfg=first, splitk=1,
                              w_f16=ops.split_weights_f16x2(wk, one), amax_in=ops.amax_slots(x))


def test_patch_3x3_is_bit_identical_to_the_f16x2_tiles():
    """csrc/conv_patch.hip (3x3 / stride 1 / pad 1, C = 32, K = 32 / 64: input patch staged once per 8 x 32-pixel output tile,
    split into its fp16 terms once) against the 128x64 f16x2 tile of conv_x3.hip -- same products in the same order, so y must be
    EQUAL; maps narrower / lower than a tile, widths and heights that are no multiples of 32 / 8, one pixel, many images (more
    tiles than workgroups), all activations, the output as a slice of a wider buffer, per-image scales far apart."""
    from ppyolo_hip import ops
    cfg = ops.patch_first_cfg()
    g = torch.Generator().manual_seed(4300)
    for N, H, W, K, act, y_extra in ((2, 24, 40, 32, 'relu', 0), (3, 9, 7, 64, 'relu', 0), (1, 1, 1, 32, None, 0), (5, 8, 33, 64, 'leaky', 64),
                                     (2, 50, 70, 32, 'relu', 32), (40, 17, 65, 64, 'relu', 0), (1, 304, 304, 32, 'relu', 0)):
        C = 32
        x = torch.randn(N, C, H, W, generator=g) * torch.exp(2 * torch.randn(N, 1, 1, 1, generator=g))
        w = torch.randn(K, C, 3, 3, generator=g) * (1.0 / (9 * C) ** 0.5)
        sc, sh = (torch.rand(K, generator=g) + 0.5).cuda(), torch.randn(K, generator=g).cuda()
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        wf = ops.split_weights_f16x2(wk, sc)
        outs, maxima = [], []
        for c in (cfg, 44):
            y = torch.full((N, H, W, K + y_extra), 9.0).cuda()
            am = ops.amax_slots(N=N, device=y.device)
            ops.conv2d_bn_act(ops.View(xd), wk, sc, sh, ops.View(y, 0, K), 1, 1, act, cfg=c, splitk=1, w_f16=wf,
                              amax_in=ops.amax_slots(xd), amax_out=am)
            torch.cuda.synchronize()
            outs.append(y)
            maxima.append(_amax_per_image(am, N))
        what = 'N%d %dx%d K%d act %s' % (N, H, W, K, act)
        ref = F.conv2d(x, w, None, 1, 1) * sc.cpu().view(1, -1, 1, 1) + sh.cpu().view(1, -1, 1, 1)
        ref = {'relu': F.relu, 'leaky': lambda t: F.leaky_relu(t, 0.1), None: lambda t: t}[act](ref)
        close(nchw(outs[0][..., :K]), ref, what=what)
        assert torch.equal(outs[0], outs[1]), what
        assert torch.equal(maxima[0], outs[0][..., :K].reshape(N, -1).abs().amax(dim=1)), what


def test_patch_3x3_refuses_what_it_cannot_run():
    from ppyolo_hip import ops
    from ppyolo_hip._lib import PPYoloHipError
    for C, K, R, stride in ((64, 64, 3, 1), (32, 96, 3, 1), (32, 32, 1, 1), (32, 32, 3, 2)):
        x = torch.randn(1, 8, 8, C).cuda()
        wk = torch.randn(K, R, R, C).cuda()
        one, zero = torch.ones(K).cuda(), torch.zeros(K).cuda()
        Ho, Wo = ops.conv_out_hw(8, 8, R, R, stride, (R - 1) // 2)
        y = torch.zeros(1, Ho, Wo, K).cuda()
        with pytest.raises(PPYoloHipError):
            ops.conv2d_bn_act(ops.View(x), wk, one, zero, ops.View(y), stride, (R - 1) // 2, None, cfg=ops.patch_first_cfg(), splitk=1,
                              w_f16=ops.split_weights_f16x2(wk, one), amax_in=ops.amax_slots(x))


KP_IDS = (9, 10, 11, 12, 13, 14, 15)      # local ids of the k-parity tiles of csrc/conv_ws.hip (128x128 with 3 / 4 stages, 64x128 with 4 / 6; two chunks per stage: 128x128, 64x128 x 2)


def test_specialised_wave_tiles_are_bit_identical_to_the_f16x2_tiles():
    """csrc/conv_ws.hip (four waves deliver operands, four multiply) against the f16x2 tiles of conv_x3.hip: same operand
    layouts, same products in the same order, same epilogue -- EQUAL outputs over 3x3 / 1x1, strides, tiny maps, tiles that
    straddle images, K not a multiple of 4 (scalar epilogue) or of the tile, shortcuts, split-K that does not divide the chunks,
    reductions shorter than the stage count."""
    from ppyolo_hip import ops
    first = ops.ws_first_cfg()
    from ppyolo_hip._lib import lib
    nws = sum(d.family in ('ws', 'ws_pre', 'kparity') for d in ops.conv_cfgs())          # (behind them: the small-output tiles of csrc/conv_small.hip, test_small_output_tiles_*)
    g = torch.Generator().manual_seed(4400)
    ws = torch.empty(16 << 20).cuda()
    for N, H, W, C, K, R, stride, res, splitk in ((2, 19, 19, 64, 136, 3, 1, True, 1), (1, 1, 1, 32, 40, 3, 1, False, 1), (3, 1, 7, 64, 72, 1, 1, True, 2),
                                                  (5, 2, 2, 96, 64, 3, 1, False, 4), (1, 33, 31, 32, 258, 3, 2, False, 2), (4, 6, 5, 160, 27, 3, 1, False, 5),
                                                  (2, 38, 38, 256, 256, 1, 1, True, 1), (2, 24, 24, 128, 256, 3, 1, False, 1), (2, 13, 11, 1024, 100, 1, 1, True, 3),
                                                  # weights outweigh the activations: the tile order is cut into column panels (conv_shared.h ppy_panel_n), differently
                                                  # per tile width -- every tile must still be computed exactly once
                                                  (2, 19, 19, 512, 1024, 1, 1, True, 1), (3, 19, 19, 256, 520, 3, 1, False, 1)):
        pad = (R - 1) // 2
        x = torch.randn(N, C, H, W, generator=g) * torch.exp(torch.randn(N, 1, 1, 1, generator=g))
        w = torch.randn(K, C, R, R, generator=g) * (1.0 / (R * R * C) ** 0.5)
        sc, sh = (torch.rand(K, generator=g) + 0.5).cuda(), torch.randn(K, generator=g).cuda()
        ref = F.conv2d(x, w, None, stride, pad) * sc.cpu().view(1, -1, 1, 1) + sh.cpu().view(1, -1, 1, 1)
        r = torch.randn(ref.shape, generator=g) if res else None
        ref = F.leaky_relu(ref + r if res else ref, 0.1)
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        rd = nhwc(r).cuda() if res else None
        wf = ops.split_weights_f16x2(wk, sc)
        Ho, Wo = ref.shape[2], ref.shape[3]
        outs = []
        for c in [41] + [first + i for i in range(nws)]:
            y = torch.full((N, Ho, Wo, K), 9.0).cuda()
            am = ops.amax_slots(N=N, device=y.device)
            ops.conv2d_bn_act(ops.View(xd), wk, sc, sh, ops.View(y), stride, pad, 'leaky', residual=None if rd is None else ops.View(rd),
                              cfg=c, splitk=splitk, ws=ws, w_f16=wf, amax_in=ops.amax_slots(xd), amax_out=am)
            torch.cuda.synchronize()
            outs.append(y)
        what = 'N%d %dx%d C%d K%d R%d s%d res %s split %d' % (N, H, W, C, K, R, stride, res, splitk)
        close(nchw(outs[0]), ref, what=what)
        for i, y in enumerate(outs[1:]):
            if i in KP_IDS:        # k-parity tiles (round 6): two k-groups summed at the end -- one more fp32 rounding, like a split-K of two
                close(nchw(y), ref, what=what + ' (k-parity tile %d)' % i)
                assert torch.equal(y, outs[1 + KP_IDS[0]]), '%s: the k-parity tiles differ from each other (same two sums, same order)' % what
            else:
                assert torch.equal(outs[0], y), '%s: ws cfg %d differs from the f16x2 tile' % (what, i)


def _small_ks(splitk, nwave, chunks):
    """k-parts csrc/conv_small.hip makes of a request: the largest power of two <= min(splitk, waves, chunks) (launch_small)."""
    ks = 1
    while 2 * ks <= splitk and 2 * ks <= nwave and 2 * ks <= chunks:
        ks *= 2
    return ks


def test_small_output_tiles_are_bit_identical_to_the_f16x2_tiles():
    """Round 6, csrc/conv_small.hip (ids ppy_conv2d_small_first_config() + 0..3: a WAVE owns a 32x32 / 32x64 output tile and one k-part,
    operands straight from the L2 into fragment registers, the k-parts of a tile added inside the workgroup) against the f16x2 tile of
    conv_x3.hip with the SAME split count: same chunk ranges, same products, same order of additions -- EQUAL outputs and equal tracked
    maxima, without a workspace.  Shapes: batch-1 maps of the R50vd / r18vd plans, tiny maps, tiles that straddle images, K not a multiple
    of 4 (scalar epilogue; conv_offset's 27) or of the tile, strides, shortcuts, 2x2 upsampling stores, a CoordConv bias map, reductions
    shorter than the request depth, more k-parts asked for than waves / chunks."""
    from ppyolo_hip import ops
    first = ops.small_first_cfg()
    assert [d.id for d in ops.conv_cfgs() if d.family == 'small'] == list(range(first, first + 4))
    NW = (4, 4, 8, 8)
    g = torch.Generator().manual_seed(6100)
    ws = torch.empty(16 << 20).cuda()
    cases = ((1, 19, 19, 512, 256, 1, 1, True, 4, False, False), (1, 19, 19, 256, 512, 3, 1, False, 8, False, False),
             (1, 38, 38, 128, 27, 3, 2, False, 8, False, False), (2, 10, 10, 64, 136, 3, 1, True, 2, False, False),
             (1, 1, 1, 32, 40, 3, 1, False, 1, False, False), (3, 1, 7, 64, 72, 1, 1, True, 2, False, False),
             (5, 2, 2, 96, 64, 3, 1, False, 4, False, False), (1, 33, 31, 32, 258, 3, 2, False, 16, False, False),
             (4, 6, 5, 160, 27, 3, 1, False, 5, False, False), (1, 19, 19, 256, 128, 1, 1, False, 2, True, False),
             (2, 13, 11, 96, 100, 1, 1, True, 3, False, True), (1, 20, 20, 64, 260, 1, 1, False, 1, False, True))
    for N, H, W, C, K, R, stride, res, splitk, ups, posb in cases:
        pad = (R - 1) // 2
        chunks = R * R * C // 32
        x = torch.randn(N, C, H, W, generator=g) * torch.exp(torch.randn(N, 1, 1, 1, generator=g))
        w = torch.randn(K, C, R, R, generator=g) * (1.0 / (R * R * C) ** 0.5)
        sc, sh = (torch.rand(K, generator=g) + 0.5).cuda(), torch.randn(K, generator=g).cuda()
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        r = torch.randn(N, Ho, Wo, K, generator=g).cuda() if res else None
        pb = (torch.randn(1, Ho, Wo, K, generator=g) * 0.3).cuda() if posb else None
        wk = w.permute(0, 2, 3, 1).contiguous().cuda()
        xd = nhwc(x).cuda()
        wf = ops.split_weights_f16x2(wk, sc)
        pbf = (pb * (sc / wf[1])).contiguous() if posb else None
        up = 2 if ups else 1

        def run(c, s, scratch):
            y = torch.full((N, up * Ho, up * Wo, K), 9.0).cuda()
            am = ops.amax_slots(N=N, device=y.device)
            ops.conv2d_bn_act(ops.View(xd), wk, sc, sh, ops.View(y), stride, pad, 'leaky', residual=None if r is None else ops.View(r),
                              posbias=pb, upsample2x=ups, cfg=c, splitk=s, ws=scratch, w_f16=wf, amax_in=ops.amax_slots(xd), amax_out=am,
                              posbias_f16=pbf)
            torch.cuda.synchronize()
            return y, am.view(N, -1).amax(dim=1)
        what = 'N%d %dx%d C%d K%d R%d s%d res %s split %d ups %s posb %s' % (N, H, W, C, K, R, stride, res, splitk, ups, posb)
        ref = F.conv2d(x, w, None, stride, pad)
        if posb:
            ref = ref + nchw(pb.cpu())
        ref = ref * sc.cpu().view(1, -1, 1, 1) + sh.cpu().view(1, -1, 1, 1)
        ref = F.leaky_relu(ref + nchw(r.cpu()) if res else ref, 0.1)
        if ups:
            ref = F.interpolate(ref, scale_factor=2, mode='nearest')
        tile = {}
        for i in range(4):
            ks = _small_ks(splitk, NW[i], chunks)
            if ks not in tile:
                tile[ks] = run(41, ks, ws)
                close(nchw(tile[ks][0]), ref, what=what)
            y, am = run(first + i, splitk, None)          # no workspace: the k-parts never leave the launch
            assert torch.equal(y, tile[ks][0]), '%s: small cfg %d (%d k-parts) differs from the f16x2 tile by %.3e' % (
                what, i, ks, float((y - tile[ks][0]).abs().max()))
            if Ho * Wo >= 64:          # (a 32-row wave tile touches at most two images: the tracked maxima are exact, common.h amax_track2)
                assert torch.equal(am, tile[ks][1]), '%s: tracked maxima differ' % what
            else:                      # tiny maps: an image behind the first of a wave tile gets an upper bound -- never less than its maximum
                true = y.abs().reshape(N, -1).amax(dim=1)
                assert torch.all(am >= true) and torch.all(am <= true.max()), '%s: tracked maxima %s vs %s' % (what, am.tolist(), true.tolist())
    assert ops.conv2d_workspace_bytes(1, 19, 19, 512, 256, 1, 1, 1, 0, first, 8) == 0


def test_small_output_tiles_read_and_write_presplit_tensors():
    """The same kernels on both sides of a pre-split link (ppy_conv2d_bn_act_split_f32): as the CONSUMER of finished operands (with
    k-parts too -- a tile kernel cannot split there) and as the PRODUCER of such a tensor, against a tile kernel in the same place: equal
    outputs for one k-part, fp32 rounding between different part counts; the stored scales are the tile's."""
    from ppyolo_hip import ops
    first, f0 = ops.small_first_cfg(), first_cfg('f16x2')
    g = torch.Generator().manual_seed(6200)
    for C, Km, K2, H, R2, stride in ((256, 128, 256, 19, 3, 1), (512, 64, 96, 12, 3, 2), (64, 256, 128, 16, 1, 1)):
        N = 3
        x = torch.relu(torch.randn(N, H, H, C, generator=g))
        x[1] *= 200.0
        x[2] *= 1e-3
        w1 = torch.randn(Km, 1, 1, C, generator=g) * (2.0 / C) ** 0.5
        w2 = torch.randn(K2, R2, R2, Km, generator=g) * (2.0 / (R2 * R2 * Km)) ** 0.5
        sc1, sh1 = torch.rand(Km, generator=g) + 0.5, torch.randn(Km, generator=g) * 0.1
        sc2, sh2 = torch.rand(K2, generator=g) + 0.5, torch.randn(K2, generator=g) * 0.1
        mul = float((sc1.abs().double() * w1.abs().double().sum(dim=(1, 2, 3))).max()) * (1 + 2.0 ** -8)
        add = float(sh1.abs().max()) * (1 + 2.0 ** -8)
        pad2 = (R2 - 1) // 2
        Ho = (H + 2 * pad2 - R2) // stride + 1
        xd, w1d, w2d = x.cuda(), w1.cuda(), w2.cuda()
        f1, f2 = ops.split_weights_f16x2(w1d, sc1.cuda()), ops.split_weights_f16x2(w2d, sc2.cuda())

        def run(pcfg, ps, ccfg, cs):
            mid = torch.zeros(N, H, H, Km).cuda()
            out = torch.zeros(N, Ho, Ho, K2).cuda()
            a_in, a_mid, a_out = ops.amax_slots(xd), ops.amax_slots(N=N, device='cuda'), ops.amax_slots(N=N, device='cuda')
            ys = (torch.ones(N).cuda(), mul, add)
            ops.conv2d_bn_act(ops.View(xd), w1d, sc1.cuda(), sh1.cuda(), ops.View(mid), 1, 0, 'relu', None, None, False, pcfg, ps,
                              None, None, f1, a_in, a_mid, None, None, ys)
            ops.conv2d_bn_act(ops.View(mid), w2d, sc2.cuda(), sh2.cuda(), ops.View(out), stride, pad2, None, None, None, False,
                              ccfg, cs, None, None, f2, a_mid, a_out, None, ys[0], None)
            torch.cuda.synchronize()
            return out, mid, ys[0].clone()
        base_out, base_mid, base_scales = run(f0 + 1, 1, f0 + 1, 1)
        for i in range(4):
            out, mid, scales = run(first + i, 1, first + i, 1)
            assert torch.equal(mid.view(torch.int32), base_mid.view(torch.int32)), 'producer cfg %d: the split tensor differs' % i
            assert torch.equal(scales, base_scales)
            assert torch.equal(out, base_out), 'consumer cfg %d differs by %.3e' % (i, float((out - base_out).abs().max()))
            out2, mid2, _ = run(first + i, 4, first + i, 8)          # k-parts on both sides of the link
            close(out2, base_out, rel=2e-6, what='C%d: k-parts on a pre-split link, cfg %d' % (C, i))


def test_stem_conv_with_maxpool_from_the_epilogue_is_the_two_launches():
    """ppy_conv3x3_maxpool_f32 (csrc/conv_patch.hip, MPOOL): conv1_3 of the stem (reference model/resnet_vd.py:110) + MaxPool2d(3, 2, 1)
    (:103, :136) in one launch against the patch kernel followed by ppy_maxpool3x3s2_f32: EQUAL outputs and equal tracked maxima -- odd
    and even sizes, maps smaller than a tile, sizes that are not multiples of the 3 x 15 pooled tile, images of very different magnitude,
    an all-zero image, ReLU / LeakyReLU / no activation (negative values: padding must behave as -inf, not 0), and the pooled
    tensor as a channel slice of a wider buffer (the first block's folded-shortcut input)."""
    from ppyolo_hip import ops
    from ppyolo_hip._lib import PPYoloHipError
    g = torch.Generator().manual_seed(3103)
    for N, H, W, act, wide in ((2, 38, 50, 'relu', False), (1, 7, 9, None, False), (3, 64, 64, 'leaky', True), (1, 1, 1, None, False),
                               (2, 13, 31, 'relu', True), (2, 30, 90, None, False), (1, 2, 2, 'leaky', False), (2, 97, 45, 'relu', False)):
        x = torch.randn(N, 32, H, W, generator=g) * torch.exp(2.0 * torch.randn(N, 1, 1, 1, generator=g))
        if N > 2:
            x[1] = 0
        w = torch.randn(64, 32, 3, 3, generator=g) * (1.0 / 288 ** 0.5)
        sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), torch.randn(64, generator=g).cuda()
        wk, xd = w.permute(0, 2, 3, 1).contiguous().cuda(), nhwc(x).cuda()
        wf = ops.split_weights_f16x2(wk, sc)
        Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        # two launches
        y = torch.empty(N, H, W, 64).cuda()
        am0 = ops.amax_slots(N=N, device=y.device)
        ops.conv2d_bn_act(ops.View(xd), wk, sc, sh, ops.View(y), 1, 1, act, cfg=ops.patch_first_cfg(), splitk=1, w_f16=wf,
                          amax_in=ops.amax_slots(xd), amax_out=am0)
        p0 = torch.empty(N, Hp, Wp, 64).cuda()
        ops.maxpool3x3s2(ops.View(y), ops.View(p0))
        # one
        buf = torch.full((N, Hp, Wp, 128 if wide else 64), 7.0).cuda()
        pv = ops.View(buf, 64, 64) if wide else ops.View(buf)
        am1 = ops.amax_slots(N=N, device=y.device)
        ops.conv3x3_maxpool(ops.View(xd), wf, sh, pv, act, amax_in=ops.amax_slots(xd), amax_out=am1)
        torch.cuda.synchronize()
        what = 'N%d %dx%d %s' % (N, H, W, act)
        got = buf[..., 64:] if wide else buf
        assert torch.equal(got, p0), '%s: %d values differ' % (what, int((got != p0).sum()))
        if wide:
            assert bool((buf[..., :64] == 7.0).all()), what + ': wrote outside its channel slice'
        assert torch.equal(am0.view(N, -1).max(dim=1).values, am1.view(N, -1).max(dim=1).values), what + ': tracked maxima'
        ref = F.max_pool2d(nchw(y), 3, 2, 1)
        assert torch.equal(nchw(p0), ref), what + ': the pooling launch itself'
    # any other geometry is refused
    x = torch.randn(1, 8, 8, 64).cuda()
    wk = torch.randn(64, 3, 3, 64).cuda()
    one = torch.ones(64).cuda()
    with pytest.raises(PPYoloHipError):
        ops.conv3x3_maxpool(ops.View(x), ops.split_weights_f16x2(wk, one), one, ops.View(torch.empty(1, 4, 4, 64).cuda()), 'relu',
                            amax_in=ops.amax_slots(x))


# ------------------------------------------------------------------------------------------
# conv2 -> conv3 of an identity bottleneck in one launch (round 5, csrc/conv_b2b.hip)
@pytest.mark.parametrize('N,H,W,pool', [(2, 19, 19, False), (3, 24, 40, False), (1, 76, 76, False), (4, 8, 8, False),
                                        (3, 24, 40, True), (1, 76, 76, True), (4, 8, 8, True), (2, 6, 10, True)])
def test_conv3x3_conv1x1_matches_two_launches_and_fp64(N, H, W, pool):
    """relu(bn3(conv3(relu(bn2(conv2(t))))) + x) with t pre-split by conv1 (reference model/resnet_vd.py:81-87), ONE launch
    (ppy_conv3x3_conv1x1_f32) against the two-launch form and float64: error vs float64 no larger than 1.5 x the two launches'
    (fp32-grade), the tracked maxima equal to max|y| per image, tiles that straddle rows / images / the end of the tensor
    (M = 722, 2880, 5776, 256), images of very different magnitude and an all-zero image.  pool: the tile's rows are 2x2 blocks and
    AvgPool2d(2, 2) of the output is written too -- bit-equal to (((a + b) + c) + d) * 0.25 of the y the same launch stored."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(23 + H)
    f0 = first_cfg('f16x2')
    C = 256
    x = torch.relu(torch.randn(N, H, W, C, generator=g))
    if N > 1:
        x[1] *= 200.0
    if N > 2:
        x[2] = 0.0
    w1 = torch.randn(64, 1, 1, C, generator=g) * (2.0 / C) ** 0.5
    w2 = torch.randn(64, 3, 3, 64, generator=g) * (2.0 / 576) ** 0.5
    w3 = torch.randn(256, 1, 1, 64, generator=g) * (2.0 / 64) ** 0.5
    sc = [torch.rand(k, generator=g) + 0.5 for k in (64, 64, 256)]
    sh = [torch.randn(k, generator=g) * 0.1 for k in (64, 64, 256)]
    t = torch.relu(torch.einsum('nhwc,kc->nhwk', x.double(), w1[:, 0, 0].double()) * sc[0].double() + sh[0].double())
    t = F.conv2d(t.permute(0, 3, 1, 2), w2.permute(0, 3, 1, 2).double(), padding=1).permute(0, 2, 3, 1)
    t = torch.relu(t * sc[1].double() + sh[1].double())
    ref = torch.relu(torch.einsum('nhwc,kc->nhwk', t, w3[:, 0, 0].double()) * sc[2].double() + sh[2].double() + x.double())

    def run(fused):
        xd = x.cuda()
        t1, t2, out = torch.zeros(N, H, W, 64).cuda(), torch.zeros(N, H, W, 64).cuda(), torch.full((N, H, W, 256), float('nan')).cuda()
        a_in, a1, a2, a_out = ops.amax_slots(xd), ops.amax_slots(N=N, device='cuda'), ops.amax_slots(N=N, device='cuda'), ops.amax_slots(N=N, device='cuda')
        wd = [w.cuda() for w in (w1, w2, w3)]
        scd, shd = [v.cuda() for v in sc], [v.cuda() for v in sh]
        fs = [ops.split_weights_f16x2(w, s_) for w, s_ in zip(wd, scd)]
        mul = float((sc[0].abs().double() * w1.abs().double().sum(dim=(1, 2, 3))).max()) * (1 + 2.0 ** -8)
        ys = (torch.ones(N).cuda(), mul, float(sh[0].abs().max()) * (1 + 2.0 ** -8))
        ops.conv2d_bn_act(ops.View(xd), wd[0], scd[0], shd[0], ops.View(t1), 1, 0, 'relu', None, None, False, f0 + 4, 1, None, None, fs[0], a_in, a1,
                          None, None, ys)
        if fused:
            tm = float((sc[1].abs().double() * w2.abs().double().sum(dim=(1, 2, 3))).max()) * (1 + 2.0 ** -8)
            pl = torch.full((N, H // 2, W // 2, 256), float('nan')).cuda() if pool else None
            ops.conv3x3_conv1x1(ops.View(t1), ys[0], a1, fs[1], shd[1], fs[2], shd[2], ops.View(xd), ops.View(out), tm,
                                float(sh[1].abs().max()) * (1 + 2.0 ** -8), a_out, None if pl is None else ops.View(pl))
            if pool:
                o = out
                want = (((o[:, 0::2, 0::2] + o[:, 0::2, 1::2]) + o[:, 1::2, 0::2]) + o[:, 1::2, 1::2]) * 0.25
                assert torch.equal(pl, want)
        else:
            ops.conv2d_bn_act(ops.View(t1), wd[1], scd[1], shd[1], ops.View(t2), 1, 1, 'relu', None, None, False, f0 + 4, 1, None, None, fs[1], a1, a2,
                              None, ys[0], None)
            ops.conv2d_bn_act(ops.View(t2), wd[2], scd[2], shd[2], ops.View(out), 1, 0, 'relu', ops.View(xd), None, False, f0 + 4, 1, None, None, fs[2],
                              a2, a_out)
        torch.cuda.synchronize()
        return out.cpu().double(), a_out.view(N, -1).amax(dim=1).cpu()
    two, mx_two = run(False)
    one, mx_one = run(True)
    assert torch.isfinite(one).all()
    for n in range(N):
        den = ref[n].abs().max().clamp_min(1e-30)
        e_two = float((two[n] - ref[n]).abs().max() / den)
        e_one = float((one[n] - ref[n]).abs().max() / den)
        assert e_one <= 1.5 * e_two + 2e-7, (n, e_one, e_two)
        assert float(mx_one[n]) == float(one[n].abs().max().float()), (n, float(mx_one[n]), float(one[n].abs().max()))
    # shapes outside the supported family are refused
    from ppyolo_hip._lib import PPYoloHipError, lib
    assert lib().ppy_conv3x3_conv1x1_f32(None, 64, None, None, None, None, None, None, None, None, None, 256, None, 256, None, 0, 1, 8, 8, 64, 64,
                                         256, 1.0, 1.0, None, None) == -1


@pytest.mark.parametrize('pool', [False, True])
def test_conv3x3_conv1x1_is_bit_repeatable_at_full_size(pool):
    """The fused launch at the R50vd-608 batch-8 shape (1444 workgroups, three rounds of two per CU), 24 times on the same inputs with
    traffic on a second stream every other run: every output bit-equal to the first.  (A version whose main loop let the last
    fragment read of a stage complete behind the workgroup barrier differed in 141 of 299 runs, by up to 3e-4 -- and by 1.3 with
    pooled rows; the small shapes above never showed it.)"""
    from ppyolo_hip import ops
    N, H, W = 8, 152, 152
    g = torch.Generator().manual_seed(1)
    x = torch.relu(torch.randn(N, H, W, 256, generator=g)).cuda()
    w1 = (torch.randn(64, 1, 1, 256, generator=g) * (2.0 / 256) ** 0.5).cuda()
    w2 = (torch.randn(64, 3, 3, 64, generator=g) * (2.0 / 576) ** 0.5).cuda()
    w3 = (torch.randn(256, 1, 1, 64, generator=g) * (2.0 / 64) ** 0.5).cuda()
    one64, one256, z64, z256 = torch.ones(64).cuda(), torch.ones(256).cuda(), torch.zeros(64).cuda(), torch.zeros(256).cuda()
    fs = [ops.split_weights_f16x2(w1, one64), ops.split_weights_f16x2(w2, one64), ops.split_weights_f16x2(w3, one256)]
    t1 = torch.zeros(N, H, W, 64).cuda()
    a_in, a1 = ops.amax_slots(x), ops.amax_slots(N=N, device='cuda')
    ys = (torch.ones(N).cuda(), float(w1.abs().double().sum(dim=(1, 2, 3)).max()) * (1 + 2.0 ** -8), 0.0)
    ops.conv2d_bn_act(ops.View(x), w1, one64, z64, ops.View(t1), 1, 0, 'relu', None, None, False, 44, 1, None, None, fs[0], a_in, a1, None, None, ys)
    tm = float(w2.abs().double().sum(dim=(1, 2, 3)).max()) * (1 + 2.0 ** -8)
    side, junk = torch.cuda.Stream(), torch.empty(64 << 20, device='cuda')
    first = None
    for r in range(24):
        out = torch.full((N, H, W, 256), float('nan')).cuda()
        pl = torch.full((N, H // 2, W // 2, 256), float('nan')).cuda() if pool else None
        a_out = ops.amax_slots(N=N, device='cuda')
        if r % 2:
            with torch.cuda.stream(side):
                junk.mul_(1.0001)
        ops.conv3x3_conv1x1(ops.View(t1), ys[0], a1, fs[1], z64, fs[2], z256, ops.View(x), ops.View(out), tm, 0.0, a_out,
                            None if pl is None else ops.View(pl))
        torch.cuda.synchronize()
        got = (out, pl, a_out.clone())
        if first is None:
            first = got
            assert torch.isfinite(out).all()
        else:
            assert torch.equal(out, first[0]), 'run %d differs from run 0 by %.3e' % (r, float((out - first[0]).abs().max()))
            assert not pool or torch.equal(pl, first[1])
            assert torch.equal(got[2].view(N, -1).amax(dim=1), first[2].view(N, -1).amax(dim=1))


@pytest.mark.parametrize('shape', [(8, 38, 38, 1024, 256, 1, 1, True), (8, 38, 38, 256, 256, 3, 1, False), (8, 19, 19, 512, 1024, 3, 1, False),
                                   (8, 76, 76, 256, 256, 3, 2, False)])
def test_k_parity_tiles_are_bit_repeatable_at_full_size(shape):
    """Round 6, the k-parity tiles of csrc/conv_ws.hip (ids ws_first + 9..12) at the R50vd-608 batch-8 shapes their table entries
    run: 16 launches on the same inputs, traffic on a second stream every other run -- every output and every tracked maximum
    bit-equal to the first (the two consumer groups meet at ONE barrier per chunk and once more for the exchange of their sums: a
    race would show here, as conv_b2b's did), equal between the 3- / 4-stage variants, and as close to a float64 convolution as
    the one-group tile of the same shape."""
    from ppyolo_hip import ops
    N, H, W, C, K, R, stride, res = shape
    g = torch.Generator().manual_seed(77)
    pad = (R - 1) // 2
    x = torch.relu(torch.randn(N, H, W, C, generator=g)) * torch.exp(torch.randn(N, 1, 1, 1, generator=g))
    w = torch.randn(K, R, R, C, generator=g) * (2.0 / (R * R * C)) ** 0.5
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), None, stride, pad).permute(0, 2, 3, 1)
    Ho, Wo = ref.shape[1], ref.shape[2]
    r = torch.randn(N, Ho, Wo, K, generator=g) if res else None
    ref = F.relu(ref + r.double() if res else ref)
    mag = ref.abs().max().item()
    x, w = x.cuda(), w.cuda()
    one, zero = torch.ones(K).cuda(), torch.zeros(K).cuda()
    wf, a_in = ops.split_weights_f16x2(w, one), ops.amax_slots(x)
    rd = r.cuda() if res else None
    side, junk = torch.cuda.Stream(), torch.empty(32 << 20, device='cuda')
    first = ops.ws_first_cfg()

    def run(cfg):
        y = torch.full((N, Ho, Wo, K), float('nan')).cuda()
        am = ops.amax_slots(N=N, device='cuda')
        ops.conv2d_bn_act(ops.View(x), w, one, zero, ops.View(y), stride, pad, 'relu', residual=None if rd is None else ops.View(rd),
                          cfg=cfg, splitk=1, w_f16=wf, amax_in=a_in, amax_out=am)
        torch.cuda.synchronize()
        return y, am.view(N, -1).amax(dim=1)
    base, base_am = run(first + 10)
    assert torch.isfinite(base).all()
    for rep in range(16):
        if rep % 2:
            with torch.cuda.stream(side):
                junk.mul_(1.0001)
        c = (9, 13, 10, 15)[rep % 4]
        y, am = run(first + c)
        assert torch.equal(y, base), 'run %d (cfg ws+%d) differs by %.3e' % (rep, c, float((y - base).abs().max()))
        assert torch.equal(am, base_am)
    plain, _ = run(first + 1)                  # the same tile with one consumer group
    e_kp = float((base.cpu().double() - ref).abs().max()) / mag
    e_plain = float((plain.cpu().double() - ref).abs().max()) / mag
    assert e_kp <= 1.5 * e_plain + 1e-7, (e_kp, e_plain)


# ------------------------------------------------------------------------------------------
# "global pre-split": a producer convolution stores its output as its one consumer's finished MFMA operands
def test_presplit_pair_matches_fp64_as_well_as_the_plain_pair():
    """1x1 (+ CoordConv bias map, LeakyReLU) -> 3x3 as in the head, and 1x1 (ReLU) -> strided 3x3 as in a bottleneck: the
    intermediate tensor travels as two fp16 terms of y * s_image with s from a STATIC bound (ppy_conv2d_bn_act_split_f32).
    Held to: error vs float64 no larger than 1.5 x the plain f16x2 pair's (which is fp32-grade), every tile family that
    reads / writes such tensors, images of very different magnitude in one batch, an all-zero image."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(17)
    f0 = first_cfg('f16x2')
    w0 = ops.ws_first_cfg()
    cases = [dict(C=256, Km=128, K2=256, H=19, stride=1, act='leaky', posb=True, pcfg=f0 + 4, ccfg=f0 + 2),
             dict(C=512, Km=128, K2=128, H=24, stride=2, act='relu', posb=False, pcfg=w0 + 2, ccfg=w0 + 8),
             dict(C=128, Km=64, K2=64, H=20, stride=1, act='relu', posb=False, pcfg=f0 + 13, ccfg=w0 + 0),
             dict(C=64, Km=256, K2=128, H=16, stride=1, act='leaky', posb=False, pcfg=w0 + 1, ccfg=f0 + 1)]
    for cs in cases:
        N, C, Km, K2, H = 4, cs['C'], cs['Km'], cs['K2'], cs['H']
        x = torch.relu(torch.randn(N, H, H, C, generator=g))
        x[1] *= 300.0
        x[2] *= 1e-3
        x[3] = 0.0
        w1 = torch.randn(Km, 1, 1, C, generator=g) * (2.0 / C) ** 0.5
        w2 = torch.randn(K2, 3, 3, Km, generator=g) * (2.0 / (9 * Km)) ** 0.5
        sc1, sh1 = torch.rand(Km, generator=g) + 0.5, torch.randn(Km, generator=g) * 0.1
        sc2, sh2 = torch.rand(K2, generator=g) + 0.5, torch.randn(K2, generator=g) * 0.1
        posb = torch.randn(1, H, H, Km, generator=g) * 0.3 if cs['posb'] else None
        # float64 reference
        t = torch.einsum('nhwc,kc->nhwk', x.double(), w1[:, 0, 0].double())
        if posb is not None:
            t = t + posb.double()
        t = t * sc1.double() + sh1.double()
        t = torch.where(t > 0, t, t * (0.1 if cs['act'] == 'leaky' else 0.0))
        ref = F.conv2d(t.permute(0, 3, 1, 2), w2.permute(0, 3, 1, 2).double(), stride=cs['stride'], padding=1)
        ref = (ref.permute(0, 2, 3, 1) * sc2.double() + sh2.double())
        Ho = ref.shape[1]

        def run(split):
            xd = x.cuda()
            mid = torch.zeros(N, H, H, Km).cuda()
            out = torch.zeros(N, Ho, Ho, K2).cuda()
            a_in, a_mid, a_out = ops.amax_slots(xd), ops.amax_slots(N=N, device='cuda'), ops.amax_slots(N=N, device='cuda')
            w1d, w2d = w1.cuda(), w2.cuda()
            f1, f2 = ops.split_weights_f16x2(w1d, sc1.cuda()), ops.split_weights_f16x2(w2d, sc2.cuda())
            pbd = posb.cuda() if posb is not None else None
            pbf = None
            if pbd is not None:
                s_w = sc1.cuda() / f1[1]
                pbf = (pbd * s_w).contiguous()
            ys = None
            if split:
                mul = float((sc1.abs().double() * w1.abs().double().sum(dim=(1, 2, 3))).max()) * (1 + 2.0 ** -8)
                add = sh1.abs().double()
                if posb is not None:
                    add = add + posb.abs().double().reshape(-1, Km).amax(0) * sc1.abs().double()
                ys = (torch.ones(N).cuda(), mul, float(add.max()) * (1 + 2.0 ** -8))
            ops.conv2d_bn_act(ops.View(xd), w1d, sc1.cuda(), sh1.cuda(), ops.View(mid), 1, 0, cs['act'], None, pbd, False, cs['pcfg'], 1,
                              None, None, f1, a_in, a_mid, pbf, None, ys)
            ops.conv2d_bn_act(ops.View(mid), w2d, sc2.cuda(), sh2.cuda(), ops.View(out), cs['stride'], 1, None, None, None, False,
                              cs['ccfg'], 1, None, None, f2, a_mid, a_out, None, ys[0] if split else None, None)
            torch.cuda.synchronize()
            return out.cpu().double(), (ys[0].cpu() if split else None), mid.cpu()
        plain, _, mid_plain = run(False)
        split, scales, _ = run(True)
        for n in range(N):
            den = ref[n].abs().max().clamp_min(1e-30)
            e_plain = float((plain[n] - ref[n]).abs().max() / den)
            e_split = float((split[n] - ref[n]).abs().max() / den)
            assert e_split <= 1.5 * e_plain + 2e-7, (cs, n, e_split, e_plain)
            if n < 3:        # the scale is a power of two that keeps the scaled maximum inside fp16, at most 2^8 below 2^14
                mx = float(mid_plain[n].abs().max()) * float(scales[n])
                assert 2.0 ** 5 <= mx < 2.0 ** 14, (cs, n, mx)
                m, e = np.frexp(float(scales[n]))
                assert m == 0.5
    # a kernel family that cannot read such tensors refuses instead of misreading them
    from ppyolo_hip._lib import PPYoloHipError
    xd = torch.zeros(1, 8, 8, 64).cuda()
    wd = torch.zeros(64, 1, 1, 64).cuda()
    one = torch.ones(64).cuda()
    with pytest.raises(PPYoloHipError):
        ops.conv2d_bn_act(ops.View(xd), wd, one, one, ops.View(torch.zeros(1, 8, 8, 64).cuda()), 1, 0, None, None, None, False, 3, 1,
                          None, None, None, None, None, None, torch.ones(1).cuda(), None)


def test_presplit_links_in_the_plan_and_same_detections(monkeypatch):
    """The R50vd plan links its bottleneck conv1 -> conv2 and head 1x1 -> 3x3 pairs; the detections equal those of the unlinked
    plan to fp32 noise, and an image's result still does not depend on the rest of the batch."""
    from conftest import build_model
    from config import PPYOLO_2x_Config
    from ppyolo_hip import synth
    cfg = PPYOLO_2x_Config()
    # (the headline shape: its layers have measured tile choices; a shape without table entries leaves the choice to the library
    # at launch time and is not linked)
    x, ims = synth.synth_images(8, 608).cuda(), synth.synth_im_size(8).cuda()
    model, _ = build_model(cfg, 0, 'cuda')
    ex = model._plans.executor(x)
    links = [op for op in ex.plan.ops if op.get('x_split') is not None]
    prods = [op for op in ex.plan.ops if op.get('y_split') is not None]
    assert len(links) >= 12 and len(links) >= len(prods) >= 12          # (a route has two readers)
    assert all(any(op['x_split'] is pr['y_split'][0] for pr in prods) for op in links)
    assert sum(op['w'].shape[1] == 3 for op in links) >= 12
    def padded(m, xx):
        d, c, k = m.forward_padded(xx, ims)
        torch.cuda.synchronize()
        return d.cpu(), c.cpu(), k.cpu()
    got = [p.cpu() for p in model(x, ims)]
    gd, gc, gk = padded(model, x)
    monkeypatch.setenv('PPYOLO_HIP_PRESPLIT', '0')
    model2, _ = build_model(cfg, 0, 'cuda')
    assert not any(op.get('x_split') is not None for op in model2._plans.executor(x).plan.ops)
    wd, wc, wk = padded(model2, x)
    monkeypatch.delenv('PPYOLO_HIP_PRESPLIT')
    for i in range(8):
        # the same detections (matched by keep index = candidate id); two rows may trade places only between scores closer than the
        # score tolerance (round 6: the k-parity tiles add one rounding per sum, and two near-tied rows of one class did swap)
        n = int(gc[i])
        assert n == int(wc[i]) and n > 1
        pos = {int(k): j for j, k in enumerate(wk[i, :n])}
        assert sorted(pos) == sorted(int(k) for k in gk[i, :n]), 'image %d: another set of detections' % i
        order = [pos[int(k)] for k in gk[i, :n]]
        a, b = gd[i, :n], wd[i, order]
        assert torch.equal(a[:, 0], b[:, 0])
        # (boxes: fp32 noise of the logits times the box side, as the headline comparison against the reference bounds it -- 2.3e-3 px
        # on a 640 x 354 box between the two plans under the round-6 table)
        assert (a[:, 1] - b[:, 1]).abs().max() <= 2e-6 and (a[:, 2:] - b[:, 2:]).abs().max() <= max(2e-3, 2e-5 * float(ims[i].max()))
        for j, o in enumerate(order):
            assert j == o or abs(float(gd[i, j, 1]) - float(wd[i, j, 1])) <= 2e-6, 'image %d: rows %d / %d out of place' % (i, j, o)
    big = x.clone()
    big[1] *= 50.0
    again = [p.cpu() for p in model(big, ims)]
    assert torch.equal(again[0], got[0])


def test_presplit_chain_bounds_from_the_tracked_maximum():
    """1x1 -> 3x3 -> 1x1 -> 3x3 with EVERY intermediate tensor pre-split (the head's runs): a link in the middle is consumer and
    producer at once and must bound its output from its input's TRACKED maximum -- static bounds multiplied along the chain
    lose ~2^6 per link and ran the fp16 operands into underflow (detections changed) before that was fixed.  Error vs float64
    <= 1.5 x the plain chain's; every link's scaled maximum stays within 2^9 of the fp16 target."""
    from ppyolo_hip import ops
    g = torch.Generator().manual_seed(23)
    N, H, chans, ks = 2, 19, [512, 256, 512, 256, 512], [1, 3, 1, 3]
    f0, w0 = first_cfg('f16x2'), ops.ws_first_cfg()
    cfgs = [f0 + 4, w0 + 1, f0 + 16, w0 + 0]
    x = torch.relu(torch.randn(N, H, H, chans[0], generator=g))
    x[1] *= 40.0
    ws, scs, shs = [], [], []
    for i, k in enumerate(ks):
        ws.append(torch.randn(chans[i + 1], k, k, chans[i], generator=g) * (2.0 / (k * k * chans[i])) ** 0.5)
        scs.append(torch.rand(chans[i + 1], generator=g) + 0.5)
        shs.append(torch.randn(chans[i + 1], generator=g) * 0.1)
    t = x.double()
    for w, sc, sh in zip(ws, scs, shs):
        t = F.conv2d(t.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2).double(), padding=(w.shape[1] - 1) // 2).permute(0, 2, 3, 1)
        t = t * sc.double() + sh.double()
        t = torch.where(t > 0, t, t * 0.1)
    ref = t

    def run(split):
        cur = x.cuda()
        amax = ops.amax_slots(cur)
        xs, mids, scales = None, [], []
        for i, (w, sc, sh) in enumerate(zip(ws, scs, shs)):
            wd, scd, shd = w.cuda(), sc.cuda(), sh.cuda()
            fw = ops.split_weights_f16x2(wd, scd)
            out = torch.zeros(N, H, H, w.shape[0]).cuda()
            a_out = ops.amax_slots(N=N, device='cuda')
            ys = None
            if split and i + 1 < len(ws):
                mul = float((sc.abs().double() * w.abs().double().sum(dim=(1, 2, 3))).max()) * (1 + 2.0 ** -8)
                ys = (torch.ones(N).cuda(), mul, float(sh.abs().max()) * (1 + 2.0 ** -8))
            ops.conv2d_bn_act(ops.View(cur), wd, scd, shd, ops.View(out), 1, (w.shape[1] - 1) // 2, 'leaky', None, None, False, cfgs[i], 1,
                              None, None, fw, amax, a_out, None, xs, ys)
            torch.cuda.synchronize()
            if ys is not None:
                scales.append((ys[0].cpu(), a_out.view(N, -1).amax(1).cpu()))
            cur, amax, xs = out, a_out, (ys[0] if ys is not None else None)
        return cur.cpu().double(), scales
    plain, _ = run(False)
    split, scales = run(True)
    for n in range(N):
        den = ref[n].abs().max()
        e_p, e_s = float((plain[n] - ref[n]).abs().max() / den), float((split[n] - ref[n]).abs().max() / den)
        assert e_s <= 1.5 * e_p + 2e-7, (n, e_s, e_p)
    for s, mx in scales:
        for n in range(N):
            assert 2.0 ** 5 <= float(s[n]) * float(mx[n]) < 2.0 ** 14, (float(s[n]), float(mx[n]))
