"""ppy_yolov3_loss_f32 (csrc/yolo_loss.hip) at its kinks and edges, through ops.yolov3_loss: the cases of tests/loss_cases.py
(whose own conditions tests/test_loss_cases.py checks on the CPU) against train_oracle.yolov3_loss + torch autograd.

Every run pads the head output and the gradient buffer to DIFFERENT multiples of 32 (NaN in the padding of the input: it is
never read; a sentinel in the padding of the gradient: it is never written), runs twice (bit-identical: the sums are reduced in
a fixed order), once more with accumulate=True on a pre-filled loss6 and once IN PLACE (dout aliasing the head output: the
kernel stages its rows in LDS, the bits are those of the separate-buffer run).

Bounds.  Versus the float32 oracle (all cases): 2e-5 of max|grad| per tensor of the loss's own split (ioup, x, y, w, h, obj,
cls; a tensor whose gradient a tie cancels to rounding noise is scaled by the cancelling terms), 2e-3 element-wise where |want| > 1e-4 max, 2e-5 relative per loss term -- the bounds of tests/test_gpu_train_ops.py.
Versus float64 (the margin cases, where float64 is the exact answer): the kernel's error is at most 4 x the float32 oracle's
own error on the same input, with a floor of 1e-7 of the maximum (one float32 rounding) under the oracle's error.
"""
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
RATIO_BOUND = 4.0
GEO = [(shape, ia) for shape in lc.GEOMETRY for ia in (False, True)]


def _nhwc_padded(t_nchw, ld, fill):
    N, nch, S, _ = t_nchw.shape
    b = torch.full((N, S, S, ld), fill, dtype=torch.float32)
    b[..., :nch] = t_nchw.permute(0, 2, 3, 1)
    return b.cuda()


def _launch(case, ob, db, loss6, accumulate=False, amax=None):
    from ppyolo_hip import ops
    out, tgt, gt, cfg, m = case
    nch = out.shape[1]
    ops.yolov3_loss(ops.View(ob, 0, nch), case.dev[0], case.dev[1], m['anchors'], m['C'], m['downsample'], m['scale_x_y'], m['ignore_thresh'],
                    m['w_iou'], m['iou_aware'], m['w_iou_aware'], ops.View(db, 0, nch), loss6, accumulate=accumulate, amax_dout=amax,
                    iou_loss_square=m['loss_square'])
    torch.cuda.synchronize()


def run_kernel(case):
    """-> (dout NCHW on the host, loss6 as float64 list) after the layout, repeatability, accumulate and in-place checks."""
    from ppyolo_hip import ops
    out, tgt, gt, cfg, m = case
    N, nch, S, _ = out.shape
    case.dev = (tgt.cuda(), gt.cuda())
    out_ld = (nch + 31) // 32 * 32
    dout_ld = out_ld + 32
    ob = _nhwc_padded(out, out_ld, float('nan'))
    ob0 = ob.clone()
    db = torch.full((N, S, S, dout_ld), SENTINEL).cuda()
    loss6 = torch.full((6,), 123.0).cuda()                                 # accumulate=False overwrites
    amax = ops.amax_slots(device='cuda', N=N)
    _launch(case, ob, db, loss6, amax=amax)
    assert torch.equal(ob.view(torch.int32), ob0.view(torch.int32))        # the input is only read
    assert (db[..., nch:] == SENTINEL).all(), 'padding columns of dout written'
    got = db[..., :nch]
    assert torch.isfinite(got).all() and torch.isfinite(loss6).all()
    # the tracked per-image maximum is exactly max|dout|
    assert torch.equal(amax.view(N, -1).amax(dim=1), got.reshape(N, -1).abs().amax(dim=1))
    # again: the same bits
    db2 = torch.full((N, S, S, dout_ld), SENTINEL).cuda()
    loss6b = torch.zeros(6).cuda()
    _launch(case, ob, db2, loss6b)
    assert torch.equal(db2, db) and torch.equal(loss6b, loss6)
    # accumulate=True on a pre-filled loss6: loss6 + this level (the product with 1 / N may be contracted into the addition)
    pre = torch.tensor([10., 20., 30., 40., 50., 60.]).cuda()
    acc = pre.clone()
    _launch(case, ob, db2, acc, accumulate=True)
    assert ((acc.double() - (pre.double() + loss6.double())).abs() <= 1.2e-7 * (pre.double() + loss6.double().abs())).all(), (acc, pre, loss6)
    # in place: gradients over the logits
    ib = ob0.clone()
    loss6c = torch.zeros(6).cuda()
    _launch(case, ib, ib, loss6c)
    assert torch.equal(ib[..., :nch], got) and torch.equal(loss6c, loss6)
    assert torch.isnan(ib[..., nch:]).all()
    return got.permute(0, 3, 1, 2).contiguous().cpu(), [float(v) for v in loss6.double().cpu()]


def check_against_float32(case, got, loss6):
    m = case.meta
    want, losses = lc.oracle(case.name, torch.float32)
    wp, gp = lc.split_grad(want, m), lc.split_grad(got, m)
    # Scale of a tensor: its max|grad| -- or, where a tie makes the terms of its elements CANCEL (identical boxes: d / d lw is
    # share * unit - (1 - share) * unit = 0 up to rounding), the size of the cancelling terms, the ties' `unit`
    scale = {k: wp[k].abs().max().item() for k in wp}
    for tie in m['ties']:
        k = lc.slice_of(m, tie['idx'][1])
        scale[k] = max(scale[k], tie['unit'])
    for k in wp:
        e = (gp[k].double() - wp[k].double()).abs().max().item()
        assert e <= 2e-5 * scale[k], '%s: d loss / d %s off by %.3e, scale %.3e' % (case.name, k, e, scale[k])
    big = want.abs() > 1e-4 * want.abs().max()
    assert ((got[big] - want[big]).abs() / want[big].abs()).max() <= 2e-3
    for j, nme in enumerate(lc.LOSS_NAMES):
        # (a term the float32 oracle evaluates to exactly 0 by cancellation has no relative scale of its own: the case names one)
        scale = abs(losses[nme]) if losses[nme] != 0.0 else m.get('loss_scale', {}).get(nme, 0.0)
        assert abs(loss6[j] - losses[nme]) <= 2e-5 * scale, (case.name, nme, loss6[j], losses[nme])
    return want


def check_against_float64(case, got, loss6):
    """-> the worst (kernel error) / (float32 oracle error) of the case, asserted <= RATIO_BOUND per tensor and per loss term."""
    m = case.meta
    g32, l32 = lc.oracle(case.name, torch.float32)
    g64, l64 = lc.oracle(case.name, torch.float64)
    p32, p64, pk = lc.split_grad(g32, m), lc.split_grad(g64, m), lc.split_grad(got, m)
    ratios = {}
    for k in p64:
        mx = p64[k].abs().max().item()
        if mx == 0.0:                                                       # (no positives of this kind: both must be exactly 0)
            assert pk[k].abs().max().item() == 0.0
            continue
        e_hip, e_ref = (pk[k].double() - p64[k]).abs().max().item(), (p32[k].double() - p64[k]).abs().max().item()
        ratios['d' + k] = e_hip / max(e_ref, 1e-7 * mx)
    for j, nme in enumerate(lc.LOSS_NAMES):
        if l64[nme] == 0.0:
            assert loss6[j] == 0.0
            continue
        ratios[nme] = abs(loss6[j] - l64[nme]) / max(abs(l32[nme] - l64[nme]), 1e-7 * abs(l64[nme]))
    worst = max(ratios, key=ratios.get)
    print('LOSS-EDGES %s: error vs float64 over the float32 oracle\'s: worst %.2f (%s);  %s'
          % (case.name, ratios[worst], worst, '  '.join('%s %.2f' % kv for kv in sorted(ratios.items()))))
    assert ratios[worst] <= RATIO_BOUND, (case.name, ratios)
    return ratios[worst]


@pytest.mark.parametrize('shape,iou_aware', GEO, ids=[lc.geometry_name(*g) for g in GEO])
def test_geometry_matrix(shape, iou_aware):
    """Margin cases at the shapes where the kernel's index arithmetic changes: Grid Sensitive, both iou_aware values, soft
    scores, positives in the first and last cell of every workgroup and on both sides of a grid row that two workgroups share,
    rows with two positives of an anchor (the IoU-aware broadcast), ignored negatives."""
    case = lc.get(lc.geometry_name(shape, iou_aware))
    got, loss6 = run_kernel(case)
    check_against_float32(case, got, loss6)
    check_against_float64(case, got, loss6)


@pytest.mark.parametrize('name', sorted(lc.SEMANTICS))
def test_semantics(name):
    """Inputs exactly on a kink, judged by the float32 oracle (torch autograd's rules: sign(0) = 0, min / max ties share 0.5,
    clamp passes the gradient at its bound, max propagates NaN)."""
    case = lc.get(name)
    m = case.meta
    got, loss6 = run_kernel(case)
    want = check_against_float32(case, got, loss6)
    # the elements the tie decides, one by one (`unit` = what a share off by 0.5 would add)
    for tie in m['ties']:
        assert abs(got[tie['idx']].item() - want[tie['idx']].item()) <= 1e-3 * tie['unit'], (name, tie, got[tie['idx']].item(), want[tie['idx']].item())
    if name == 'degenerate':
        for n, a, h, w in m['nan_cells']:                                  # NaN in the ignore mask's maximum: no negative term
            assert got[n, lc.channel(m, a, 4), h, w].item() == 0.0
    if name == 'disjoint':
        gp, wp = lc.split_grad(got, m), lc.split_grad(want, m)
        for k in 'wh':                                                     # clamp gate 0: only the L1 part is left, sign * ts / N
            assert torch.equal(gp[k], wp[k])
