"""ppy_dcnv2_backward_f32 / dcn_sample_bwd_kernel (csrc/dcn.hip) where random offsets never land -- zero offsets (the training's
initial state: every position an integer, border taps exactly ON the clamp bounds), integer / half-integer positions, offsets
exactly on and exactly one pixel beyond each bound, every sample colliding on four pixels, padded leading dimensions -- through
ops.dcnv2_backward against the cases and oracle of tests/dcn_cases.py (tests/test_dcn_cases.py checks those on the CPU).  And one
forward identity that does not go through the sampling restatement: zero offsets and mask 1 make DCNv2 a plain convolution.

Bounds.  Versus the float32 oracle: 2e-5 of each tensor's maximum (the bound of the golden-g15 test).  Versus float64: the
kernel's error is at most 4 x the float32 oracle's own error on the same input (floor: 1e-7 of the maximum under the oracle's).
"""
import pytest
import torch
import torch.nn.functional as F

import dcn_cases as dc

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
RATIO_BOUND = 4.0


def _padded(t_nchw, ld, fill):
    N, C, H, W = t_nchw.shape
    b = torch.full((N, H, W, ld), fill, dtype=torch.float32)
    b[..., :C] = t_nchw.permute(0, 2, 3, 1)
    return b.cuda()


def run_backward(case, x_pad=0, dx_pad=0, om_ld=27, dom_ld=27, dy_pad=0):
    """-> dict(dx, dom, dw) on the host in the oracle's layouts; padding columns hold NaN (inputs) / a sentinel (outputs) and are
    asserted untouched."""
    from ppyolo_hip import ops
    N, H, W, C, K, stride = case['shape']
    Ho, Wo = dc.out_hw(H, W, stride)
    xb, omb, dyb = _padded(case['x'], C + x_pad, float('nan')), _padded(case['om'], om_ld, float('nan')), _padded(case['dy'], K + dy_pad, float('nan'))
    keep = [t.clone() for t in (xb, omb, dyb)]
    w = case['w'].cuda()
    dx = torch.full((N, H, W, C + dx_pad), SENTINEL).cuda()
    dom = torch.full((N, Ho, Wo, dom_ld), SENTINEL).cuda()
    dw = torch.full_like(w, float('nan'))
    ops.dcnv2_backward(ops.View(xb, 0, C), w, ops.View(omb, 0, 27), ops.View(dyb, 0, K), ops.View(dx, 0, C), ops.View(dom, 0, 27), dw, stride, dc.PAD)
    torch.cuda.synchronize()
    for a, b in zip((xb, omb, dyb), keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))               # inputs only read
    assert (dx[..., C:] == SENTINEL).all(), 'dx columns >= C written'
    assert (dom[..., 27:] == SENTINEL).all(), 'd offset_mask columns 27.. written'
    got = dict(dx=dx[..., :C].permute(0, 3, 1, 2).cpu(), dom=dom[..., :27].permute(0, 3, 1, 2).cpu(), dw=dw.cpu())
    assert all(torch.isfinite(v).all() for v in got.values())
    return got


def check(name, got, group):
    """Both bounds for the three tensors; the zero pattern of the offset gradient (clamp gates) as the g15 test checks it."""
    r32, r64 = dc.oracle(name, torch.float32), dc.oracle(name, torch.float64)
    ratios = {}
    for k in ('dx', 'dom', 'dw'):
        mx = r64[k].abs().max().item()
        e32 = (got[k].double() - r32[k].double()).abs().max().item()
        assert e32 <= 2e-5 * r32[k].abs().max().item(), '%s: %s off the float32 oracle by %.3e of its maximum' % (name, k, e32 / r32[k].abs().max().item())
        e_hip, e_ref = (got[k].double() - r64[k]).abs().max().item(), (r32[k].double() - r64[k]).abs().max().item()
        ratios[k] = e_hip / max(e_ref, 1e-7 * mx)
    print('DCN-EDGES %s %s: error vs float64 over the float32 oracle\'s: %s' % (group, name, '  '.join('%s %.2f' % kv for kv in sorted(ratios.items()))))
    assert torch.equal(got['dom'][:, :18] == 0, r32['dom'][:, :18] == 0), name
    assert max(ratios.values()) <= RATIO_BOUND, (name, ratios)


@pytest.mark.parametrize('name', [n for n in dc.CASES if n.startswith('zero')])
def test_zero_offsets(name):
    """conv_offset's initial state.  The taps exactly on the lower clamp bound carry the oracle's NON-zero offset gradient (the
    gate is inclusive, as torch.clamp's backward); the engine's dom_ld = 32 with 27 columns written."""
    case = dc.get(name)
    N, H, W, C, K, stride = case['shape']
    got = run_backward(case, om_ld=32, dom_ld=32)
    check(name, got, 'zero offsets')
    py, px, ymax, xmax = dc.positions(case)
    want = dc.oracle(name)['dom']
    Ho, Wo = dc.out_hw(H, W, stride)
    g, o = (t[:, :18].permute(0, 2, 3, 1).reshape(N, Ho, Wo, 9, 2) for t in (got['dom'], want))
    for d, p, mx in ((0, py, ymax), (1, px, xmax)):
        on = (p == 0) | (p == mx)
        assert (o[..., d][p == 0] != 0).any()
        assert ((g[..., d][on] - o[..., d][on]).abs() <= 2e-5 * want.abs().max()).all()
        assert torch.equal(g[..., d][on] != 0, o[..., d][on] != 0)


@pytest.mark.parametrize('name', [n for n in dc.CASES if n.startswith('exact')])
def test_exact_positions(name):
    """Integer and half-integer offsets, offsets landing exactly on each bound (gradient passed) and exactly 1 px beyond (gate 0:
    the gradient is exactly 0 -- the zero pattern equals the oracle's)."""
    case = dc.get(name)
    got = run_backward(case)
    check(name, got, 'exact positions')
    N, H, W, C, K, stride = case['shape']
    py, px, ymax, xmax = dc.positions(case)
    Ho, Wo = dc.out_hw(H, W, stride)
    g = got['dom'][:, :18].permute(0, 2, 3, 1).reshape(N, Ho, Wo, 9, 2)
    assert not g[..., 0][(py < 0) | (py > ymax)].any() and not g[..., 1][(px < 0) | (px > xmax)].any()


def test_collisions():
    """Every tap of every output pixel steered to one fractional position: 729 atomics per channel on each of four pixels.  (The
    order of the atomics is free: no repeatability is asserted for dx.)"""
    name = [n for n in dc.CASES if n.startswith('collide')][0]
    check(name, run_backward(dc.get(name)), 'collisions')


@pytest.mark.parametrize('name', [n for n in dc.CASES if n.startswith('layout')])
def test_padded_leading_dimensions(name):
    """x_ld = C + 32, dx_ld = C + 64, om_ld = dom_ld = 32, dy_ld = K + 8, sentinels in every padding column; C = 96 (ragged last
    trip of the 64-lane loop) and C = 320 (second trip of the 256-wide gather)."""
    case = dc.get(name)
    check(name, run_backward(case, x_pad=32, dx_pad=64, om_ld=32, dom_ld=32, dy_pad=8), 'layout')


@pytest.mark.parametrize('shape', [(2, 9, 9, 64, 33, 1), (2, 10, 8, 64, 64, 2)])
def test_forward_with_zero_offsets_and_mask_one_is_a_plain_convolution(shape):
    """Zero offsets, mask logit 40 (sigmoid exactly 1 in float32): DCNv2 is F.conv2d.  Every fused configuration id x split-K in
    {1, 3} against the float64 convolution with the same scale / shift / leaky epilogue, 2e-6 of max|y| (the fused-forward test's
    bound)."""
    from ppyolo_hip import ops
    N, H, W, C, K, stride = shape
    case = dc.make('forward', shape, seed=240 + stride, offsets='zero', mask='one')
    Ho, Wo = dc.out_hw(H, W, stride)
    g = torch.Generator().manual_seed(7)
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    ref = F.conv2d(case['x'].double(), case['w'].permute(0, 3, 1, 2).double(), None, stride, dc.PAD)
    # (H + 2p - 2) // stride output rows (reference custom_layers.py:567-568): at most the convolution's
    ref = ref[:, :, :Ho, :Wo] * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = torch.where(ref > 0, ref, 0.1 * ref).permute(0, 2, 3, 1)
    x, om, w, scale, shift = _padded(case['x'], C, 0.0), _padded(case['om'], 27, 0.0), case['w'].cuda(), scale.cuda(), shift.cuda()
    w3, wf, amax = ops.split_weights_bf16x3(w), ops.split_weights_f16x2(w, scale), ops.amax_slots(x)
    worst = {}
    for cfg in range(ops.dcnv2_num_configs()):
        for splitk in (1, 3):
            need = ops.dcnv2_workspace_bytes(N, H, W, C, K, stride, dc.PAD, cfg, splitk)
            ws = torch.empty(max(need // 4, 1), device='cuda')
            y = torch.full((N, Ho, Wo, K), float('nan'), device='cuda')
            ops.dcnv2(ops.View(x), w, scale, shift, ops.View(om), ops.View(y), stride, dc.PAD, 'leaky', ws, cfg=cfg, splitk=splitk,
                      w_x3=w3, w_f16=wf, amax_in=amax, amax_out=ops.amax_slots(device='cuda', N=N))
            err = float((y.double().cpu() - ref).abs().max() / ref.abs().max())
            worst[ops.dcnv2_scheme(cfg)] = max(worst.get(ops.dcnv2_scheme(cfg), 0.0), err)
            assert err <= 2e-6, (cfg, splitk, err)
    print('DCN-EDGES forward identity %s: max error relative to max|y| per scheme: %s' % (shape, {k: '%.1e' % v for k, v in worst.items()}))
