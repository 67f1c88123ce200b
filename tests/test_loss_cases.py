"""The builders of tests/loss_cases.py keep their own promises (CPU): the margin cases stay clear of every kink in float64 with
no cell left out, the tie cases show the intended pattern in the float32 oracle's autograd and the tie decides a gradient
element large enough that a wrong share breaks the tensor-level bound of tests/test_gpu_loss_edges.py."""
import pytest
import torch

import loss_cases as lc

GEO = [(shape, ia) for shape in lc.GEOMETRY for ia in (False, True)]


@pytest.mark.parametrize('shape,iou_aware', GEO, ids=[lc.geometry_name(*g) for g in GEO])
def test_margin_cases_keep_their_distance_from_every_kink(shape, iou_aware):
    case = lc.get(lc.geometry_name(shape, iou_aware))
    out, tgt, gt, cfg, m = case
    N, S, an, C = shape
    assert tuple(out.shape) == (N, an * (5 + C) + (an if iou_aware else 0), S, S) and tuple(tgt.shape) == (N, an, 6 + C, S, S)
    assert cfg.head['num_classes'] == C and len(cfg.head['anchor_masks'][0]) == an and cfg.head['iou_aware'] == iou_aware
    assert cfg.yolo_loss['scale_x_y'] == 1.05                                     # Grid Sensitive
    r = lc.margins(case)                                                          # minima over ALL cells: nothing is excluded
    assert r['n_nan'] == 0
    assert r['ignore'] >= 1e-4 and r['xy'] >= 1e-4 and r['wh'] >= 1e-4 and r['iou'] >= 1e-5, r
    # what the case is for: positives at the workgroup edges, soft scores, ignored and counted negatives, the broadcast
    cells = S * S
    pos = {(n, h * S + w) for n, a, h, w in m['positives']}
    for n in range(N):
        want = {0, min(63, cells - 1), cells - 1} | {c for k in range(1, (cells - 1) // 64 + 1) for c in (64 * k - 1, 64 * k)}
        assert {(n, c) for c in want} <= pos
    assert r['n_positives'] == len(m['positives']) and r['n_soft_scores'] >= 1
    assert r['n_ignored_negatives'] >= 1 and r['n_counted_negatives'] >= 1
    if S > 1:
        assert r['n_broadcast_rows'] >= 1                                         # T > tobj somewhere
        assert (r['n_iou_aware_only'] >= 1) == iou_aware                          # tobj = 0 in a row with T != 0
    if cells > 64:                                                                # a grid row in two workgroups, positives on both sides
        assert 64 % S != 0 and {(0, 63), (0, 64)} <= pos
    # float32 and float64 agree on the ignore mask (so float64 is the exact answer of THIS input)
    g32, l32 = lc.oracle(case.name, torch.float32)
    g64, l64 = lc.oracle(case.name, torch.float64)
    assert torch.isfinite(g32).all() and torch.isfinite(g64).all()
    for k in lc.LOSS_NAMES:
        assert abs(l32[k] - l64[k]) <= 1e-5 * abs(l64[k]), (k, l32[k], l64[k])
    assert (g32.double() - g64).abs().max() <= 1e-5 * g64.abs().max()
    assert (l64['loss_iou_aware'] != 0.0) == iou_aware


def test_geometry_matrix_reaches_the_class_split_edges():
    """n0 = C / 10, per = ceil((C - n0) / 3) over the four class waves: empty, ragged and single-class parts all occur."""
    parts = {}
    for N, S, an, C in lc.GEOMETRY:
        n0 = C // 10
        per = (C - n0 + 2) // 3
        parts[C] = [n0] + [min(C, n0 + q * per) - min(C, n0 + (q - 1) * per) for q in (1, 2, 3)]
        assert sum(parts[C]) == C
    assert parts[1] == [0, 1, 0, 0] and parts[3] == [0, 1, 1, 1] and parts[9] == [0, 3, 3, 3]
    assert parts[11] == [1, 4, 4, 2] and parts[20] == [2, 6, 6, 6] and parts[91] == [9, 28, 28, 26] and parts[300] == [30, 90, 90, 90]
    assert any(an == 4 for _, _, an, _ in lc.GEOMETRY) and {1, 2, 3, 4} == {an for _, _, an, _ in lc.GEOMETRY}


@pytest.mark.parametrize('name', sorted(lc.SEMANTICS))
def test_tie_cases_show_their_pattern_in_the_float32_autograd(name):
    case = lc.get(name)
    out, tgt, gt, cfg, m = case
    grad, losses = lc.oracle(name, torch.float32)
    assert torch.isfinite(grad).all() and all(torch.isfinite(torch.tensor(v)) for v in losses.values())
    r = lc.margins(case)
    assert r['ignore'] >= 1e-4                      # the kinks a case is NOT about stay at a distance
    gmax = grad.abs().max().item()
    if not name.startswith('saturation'):
        assert m['ties']
    term_grads = {}
    for tie in m['ties']:
        tg = term_grads.setdefault(tie['term'], lc.term_grad(name, tie['term']))
        got = tg[tie['idx']].item()
        if tie['exact']:
            assert got == tie['want'], (tie, got)
        else:
            assert abs(got - tie['want']) <= 1e-4 * tie['unit'], (tie, got)
        # a share off by 0.5 (a gate off by 1) moves this element by `unit`: far above 2e-5 of the tensor's maximum
        assert tie['unit'] >= 1e-2 * gmax, (tie, gmax)
    body, (x, y, w, h, obj), (tx, ty, tw, th, tscale, tobj) = lc._decoded(case, torch.float32)
    pos = tscale * tobj > 0
    anchors = [v for a in m['anchors'] for v in a]
    box = lambda: (lc.trn.bbox_transform(x, y, w, h, anchors, 32, False, m['scale_x_y']), lc.trn.bbox_transform(tx, ty, tw, th, anchors, 32, True, m['scale_x_y']))
    if name == 'wh_tie':
        assert torch.equal(w[pos], tw[pos]) and torch.equal(h[pos], th[pos]) and losses['loss_wh'] == 0.0
        # one element by hand: d loss_wh / d lw = sign(lw - tw) * ts / N = 0, not ts / N
        n, a, hh, ww = m['positives'][0]
        assert term_grads['loss_wh'][n, lc.channel(m, a, 2), hh, ww].item() == 0.0 * lc._ts(case, n, a, hh, ww) / m['N']
    if name == 'xy_tie':
        px = m['scale_x_y'] * torch.sigmoid(x) - 0.5 * (m['scale_x_y'] - 1.0)
        assert torch.equal(px[pos], tx[pos]) and losses['loss_xy'] == 0.0
    if name.startswith('identical'):
        (x1, y1, x2, y2), (x1g, y1g, x2g, y2g) = box()
        for p, q in ((x1, x1g), (y1, y1g), (x2, x2g), (y2, y2g)):
            assert torch.equal(p[pos], q[pos])                   # all four ties, bit for bit
        # by hand: share s gives d loss_iou / d lw = -|d loss / d k| * (2 s - 1) / N; torch's s = 0.5 -> 0 (a share of 1 -> -2 units)
        n, a, hh, ww = m['positives'][0]
        assert abs(term_grads['loss_iou'][n, lc.channel(m, a, 2), hh, ww].item()) <= 1e-4 * m['ties'][0]['unit']
    if name == 'degenerate':
        (x1, y1, x2, y2), _ = box()
        deg = w == lc.DEGENERATE_LOGIT
        assert (deg & pos).sum() >= 4 and torch.equal(x1[deg], x2[deg]) and torch.equal(y1[deg], y2[deg])
        assert r['n_nan'] >= len(m['nan_cells']) == 6
        # the NaN of 0 / 0 reaches the mask in the float32 oracle: no objectness gradient at those negatives, where
        # sigmoid(2) / N would be the gradient of a counted negative
        for n, a, hh, ww in m['nan_cells']:
            assert tobj[n, a, hh, ww] == 0 and grad[n, lc.channel(m, a, 4), hh, ww] == 0.0
        assert not gt[0, 0].eq(0).all() and gt[0, -1].eq(0).all() and gt[1, 0].eq(0).all() and not gt[1, -1].eq(0).all()
    if name == 'disjoint':
        (x1, y1, x2, y2), (x1g, y1g, x2g, y2g) = box()
        iw, ih = torch.min(x2, x2g) - torch.max(x1, x1g), torch.min(y2, y2g) - torch.max(y1, y1g)
        assert (iw[pos] < 0).all() and (ih[pos] < 0).any() and (ih[pos] > 0).any()
        tg = lc.split_grad(term_grads['loss_iou'], m)
        for k in 'xywh':
            assert torch.equal(tg[k], torch.zeros_like(tg[k]))   # the IoU gradient is exactly zero
    if name.startswith('saturation'):
        s = torch.sigmoid(out)
        assert (s[out == 90.0] == 1.0).all() and (s[out == -90.0] == 0.0).all()
        assert min((out == v).sum().item() for v in lc.SATURATED) >= 8
        for part, t in lc.split_grad(out, m).items():            # every kind of logit the kernel takes a sigmoid of, but w / h
            assert ((t.abs() == 90.0).any() and (t.abs() == 40.0).any()) == (part not in 'wh'), part
