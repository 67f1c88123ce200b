"""The builders of tests/decode_cases.py, checked by the oracle alone (no device): every case is what it says it is, so that
tests/test_gpu_decode_edges.py judges the kernels and not the inputs.

The threshold band (|score64 / thr - 1| <= RATIO_BOUND * e32) holds at most BAND_CAP = 1e-4 of a case's pairs, ladder slots
not counted: the ladder is BUILT on the boundary (class logits at logit(thr / conf64) + d down to d = 0 under confidences
within +-500 ulps of thr), so a few thousand of its 4000 slots sit inside the band by construction -- measured 1512
(IoU-aware) and 1094 (plain) of 38880 pairs, which no cap of 1e-4 (3.9 pairs) can hold.  The builder lists them
(`ladder_band`), their number is pinned here, and on the device they are held by the assertions that need no band: list-only
candidates == candidates of the dense call, key == key of the dense score, dense score within RATIO_BOUND x e32 of float64.
"""
import numpy as np
import pytest
import torch

import decode_cases as dc

LAYOUT_NAMES = sorted(dc.LAYOUTS)
EDGE_NAMES = sorted(dc.EDGES)


def _pair(name):
    return dc.oracle(name, torch.float32), dc.oracle(name, torch.float64)


def test_the_parameter_space_is_covered():
    cases = [dc.get(n) for n in LAYOUT_NAMES]
    assert {(c.A, c.C, c.iou_aware) for c in cases} == {(3, 80, True), (3, 80, False), (3, 1, True), (1, 80, False), (2, 20, False),
                                                        (4, 7, True), (8, 3, True), (3, 85, False)}
    assert {S for c in cases for S in c.sizes} == {1, 5, 9, 13}
    assert {c.N for c in cases} == {1, 2, 3}
    assert sorted(tuple(c.sizes) for c in cases if len(c.sizes) > 1) == [(5, 9), (5, 9, 13)]
    coco = [c for c in cases if (c.A, c.C) == (3, 80)]                    # the layout that alone reaches the streaming kernel
    for group in (cases, coco):
        assert {c.scale_x_y for c in group} == {1.0, 1.05, 1.2}
        assert {c.factor for c in group if c.iou_aware} == {0.0, 0.4, 1.0}
        assert {c.clip for c in group} == {True, False}
        assert {c.thr for c in group} == {dc.f32(0.01), dc.f32(0.3)}
    assert max(c.nch for c in cases) == 270
    for c in cases:
        assert torch.equal(c.im_size, torch.tensor(dc.IM_SIZES[:c.N]))
        assert all(o.dtype == torch.float32 and o.shape == (c.N, c.nch, S, S) for o, S in zip(c.outs, c.sizes))
    assert all(dc.get(n).C in (1, 20) for n in dc.NMS_CASES)


@pytest.mark.parametrize('name', LAYOUT_NAMES)
def test_layout_case(name):
    """Candidate share in its range; float32 and float64 agree on every branch: the two IoU-aware clamps, the four clip
    comparisons, the threshold; everything finite."""
    c = dc.get(name)
    (b32, s32), (b64, s64) = _pair(name)
    assert b32.shape == (c.N, c.M, 4) and s32.shape == (c.N, c.M, c.C) and b32.dtype == torch.float32 and b64.dtype == torch.float64
    assert torch.isfinite(b64).all() and torch.isfinite(s64).all() and torch.isfinite(b32).all()
    share = (s64 > c.thr).double().mean().item()
    assert share == c.meta['share'] and 0.3 <= share <= 0.7, share
    assert torch.equal(s32 > c.thr, s64 > c.thr)
    if c.iou_aware and len(c.outs) == 1:
        for m32, m64 in zip(dc.iou_branches(c, torch.float32), dc.iou_branches(c, torch.float64)):
            assert torch.equal(m32, m64)
    u32, u64 = dc.unclipped(name, torch.float32), dc.unclipped(name, torch.float64)
    im32 = torch.stack([c.im_size[:, 1], c.im_size[:, 0]], 1)[:, None, :]
    assert torch.equal(u32[..., :2] < 0, u64[..., :2] < 0)
    assert torch.equal(u32[..., 2:] > im32, u64[..., 2:] > im32.double())
    assert dc.normal_scores(name).all()


def test_all_pass_overflows_both_lists():
    c = dc.get(dc.ALL_PASS)
    s64 = dc.oracle(dc.ALL_PASS, torch.float64)[1]
    per_image = (s64 > c.thr).flatten(1).sum(1)
    assert (per_image > 0.99 * c.M * c.C).all()
    assert c.sizes == [9] and 64 * c.A * c.C > 1536 and 16 * c.A * c.C > 768          # one workgroup's / one group's pairs


@pytest.mark.parametrize('name', dc.names())
def test_band_share_is_within_its_cap(name):
    c = dc.get(name)
    bd = dc.band(name)
    if 'ladder' in c.meta['slots']:
        lm = dc.slot_mask(name, 'ladder')
        n_ladder = int((bd & lm).sum())
        print('DECODE-CASES %s: %d of %d ladder slots inside the band (e32 %.3e)' % (name, n_ladder, int(lm.sum()), dc.e32(name)))
        # (measured: 1512 / 1094.  At most the steps with conf > thr, 100 x 20 slots, can score this near the threshold, and
        # of those only the slots with |d| (conf / thr - 1) inside the band; e32 is asserted <= 1e-6 below)
        assert 0 < n_ladder < int(lm.sum()) // 2
        bd = bd & ~lm
    assert int(bd.sum()) <= dc.BAND_CAP * c.pairs, (name, int(bd.sum()))
    assert dc.e32(name) <= 1e-6
    # outside the band the two precisions decide alike (the thr_* cases have no band: float32 decides there)
    if name not in dc.NO_BAND:
        (_, s32), (_, s64) = _pair(name)
        assert not (((s32 > c.thr) != (s64 > c.thr)) & ~dc.band(name)).any()


@pytest.mark.parametrize('name', ['ladder_ia', 'ladder_plain'])
def test_ladder(name):
    c = dc.get(name)
    (_, s32), (_, s64) = _pair(name)
    conf = c.meta['ladder_conf64']
    ulp = float(np.spacing(np.float32(c.thr)))
    assert (conf <= c.thr).sum() >= 50 and (conf > c.thr).sum() >= 50                 # both sides, conf <= thr included
    assert 300 * ulp <= (conf - c.thr).abs().max().item() <= 700 * ulp                # about +-500 ulps of conf around thr
    assert torch.equal(conf, torch.sort(conf)[0]) or torch.equal(conf, torch.sort(conf, descending=True)[0])
    o = c.outs[0][0].permute(1, 2, 0).reshape(-1, c.nch)
    obj = np.array([o[q // c.A, c.channel(q % c.A, 4)].item() for q in range(dc.LADDER_LEN)], dtype=np.float32)
    assert (np.abs(np.diff(obj.view(np.int32))) == 1).all()                           # consecutive float32 values
    lm = dc.slot_mask(name, 'ladder')
    assert int(lm.sum()) == dc.LADDER_LEN * 20
    above, below = int((s64[lm] > c.thr).sum()), int((s64[lm] <= c.thr).sum())
    assert above >= 500 and below >= 500
    # per step above the threshold: the slots at +d pass in float64, those at -d do not, +-80 / +-inf decide as 1 / 0, NaN fails
    d = torch.tensor(dc.LADDER_D, dtype=torch.float64)
    for q in range(dc.LADDER_LEN):
        row = s64[0, c.box(q // c.A, q % c.A), :20]
        assert torch.isnan(row[19]) and not torch.isnan(row[:19]).any()
        if conf[q] > c.thr * (1 + 1e-6):
            assert (row[:15][d >= 0.02] > c.thr).all() and not (row[:15][d <= -0.02] > c.thr).any()
            assert row[15] > c.thr and row[17] > c.thr and row[16] <= c.thr and row[18] == 0.0
        if conf[q] <= c.thr:
            assert not (row[:19] > c.thr).any()


def test_iou_clamps():
    c = dc.get('iou_clamps')
    f32, s32 = dc.iou_branches(c, torch.float32)
    f64, s64 = dc.iou_branches(c, torch.float64)
    assert torch.equal(f32, f64) and torch.equal(s32, s64)
    kink = -np.log(1e-7)
    first, second = {True: 0, False: 0}, {True: 0, False: 0}
    for n, b, x in c.meta['slots']['clamp']:
        if x < 0:
            assert bool(f64[n, b]) == (x < -kink) and not s64[n, b]
            first[bool(f64[n, b])] += 1
            assert abs(1.0 / (1.0 + np.exp(-x)) / 1e-7 - 1.0) >= 1e-3
        else:
            assert bool(s64[n, b]) == (x > kink) and not f64[n, b]
            second[bool(s64[n, b])] += 1
            assert abs(np.exp(-x) / 1e-7 - 1.0) >= 1e-3
    assert min(first.values()) >= 4 and min(second.values()) >= 4
    conf32 = dc.conf_of(c, torch.float32)
    for n, b, x in c.meta['slots']['clamp']:
        if s64[n, b]:
            assert conf32[n, b].item() == torch.sigmoid(-torch.log(torch.tensor(1e-7))).item()        # the saturated logit
        if f64[n, b]:
            assert abs(conf32[n, b].item() / 1e-7 - 1.0) < 1e-5


@pytest.mark.parametrize('name', [n for n in EDGE_NAMES if n.startswith('box_')])
def test_box_extremes(name):
    c = dc.get(name)
    (b32, s32), (b64, _) = _pair(name)
    sl = c.meta['slots']
    for n, b in sl['overflow']:
        if c.clip:             # x0 = -inf -> x0 * 0 = NaN; x1 = +inf -> im_w
            assert torch.isnan(b32[n, b, :2]).all() and torch.equal(b32[n, b, 2:], c.im_size[n].flip(0))
        else:
            assert torch.isinf(b32[n, b]).all() and (b32[n, b, :2] < 0).all() and (b32[n, b, 2:] > 0).all()
        assert torch.isfinite(b64[n, b]).all()                                        # float64 does not overflow at 100
    for n, b in sl['overflow_w']:
        assert not torch.isfinite(b32[n, b, 0]) and torch.isfinite(b32[n, b, 1]) and torch.isfinite(b32[n, b, 3])
    for n, b in sl['huge']:
        assert torch.isfinite(b32[n, b]).all()
        if not c.clip:
            assert b32[n, b, 2] > 1e35 and b32[n, b, 0] < -1e35
        else:
            assert b32[n, b, 0] == 0 and torch.signbit(b32[n, b, 0]) and b32[n, b, 2] == c.im_size[n, 1]      # the reference's -0.0
    for n, b in sl['tiny']:
        assert torch.isfinite(b32[n, b]).all() and (b32[n, b, 2:] - b32[n, b, :2]).abs().max() < 1e-3
    u32, u64 = dc.unclipped(name, torch.float32), dc.unclipped(name, torch.float64)
    for u in (u32, u64):
        for n, b in sl['out_left']:
            assert u[n, b, 2] < 0
        for n, b in sl['out_top']:
            assert u[n, b, 3] < 0
        for n, b in sl['out_right']:
            assert u[n, b, 0] > c.im_size[n, 1]
        for n, b in sl['out_bottom']:
            assert u[n, b, 1] > c.im_size[n, 0]
    for n, b in sl['xy_hi_lo'] + sl['xy_lo_hi']:
        assert torch.isfinite(b32[n, b]).all()
    for n, b in sl['nan_cell']:
        assert torch.isnan(b32[n, b]).all() and torch.isnan(s32[n, b]).all()
    assert len(sl['nan_conf']) == (2 if c.iou_aware else 1)
    for n, b in sl['nan_conf']:            # torch.clamp propagates the NaN through the IoU-aware re-encoding
        assert torch.isfinite(b32[n, b]).all() and torch.isnan(s32[n, b]).all()
    # tw / th stay away from the overflow point of float32 exp (88.72): a device exp overflows where torch's does
    o = c.outs[0]
    for a in range(c.A):
        wh = o[:, c.channel(a, 2):c.channel(a, 4)]
        wh = wh[torch.isfinite(wh)]
        assert ((wh - 88.72).abs() > 5).all() and ((wh + 87.3).abs() > 5).all()
    nonfinite = ~torch.isfinite(b32)
    assert int(nonfinite.sum()) >= 8


@pytest.mark.parametrize('name', dc.NO_BAND)
def test_thresholds(name):
    c = dc.get(name)
    (_, s32), (_, s64) = _pair(name)
    sl = c.meta['slots']
    (n, b, k), = sl['neg_inf']
    assert s32[n, b, k] == 0 and not torch.signbit(s32[n, b, k]) and s64[n, b, k] == 0
    (n, b, k), = sl['underflow']
    assert s32[n, b, k] == 0 and not torch.signbit(s32[n, b, k]) and s64[n, b, k] > 0          # float64 does not underflow
    (n, b, k), = sl['nan']
    assert torch.isnan(s32[n, b, k])
    (n, b, k), = sl['pos_inf']
    assert s32[n, b, k] > 0
    cand = s32 > c.thr
    total = c.pairs
    if c.thr < 0:            # every score that is not NaN, +0 included
        assert int(cand.sum()) == total - 1 and cand[sl['neg_inf'][0]] and cand[sl['underflow'][0]]
    elif c.thr == 0:
        assert int(cand.sum()) == total - 3 and not cand[sl['neg_inf'][0]] and not cand[sl['underflow'][0]]
    else:
        assert c.thr == 1.0 and int(cand.sum()) == 0
        if not c.iou_aware:
            assert s32[sl['saturated'][0]] == 1.0                                      # the largest score there is: 1 > 1 is false
    assert not torch.isnan(s32).sum() > 1


def test_float32_oracle_equals_golden_g4_bit_for_bit(golden):
    g = golden('g4_decode')
    im_size = torch.from_numpy(g['im_size'])
    for i in range(3):
        meta = [int(v) for v in g['l%d_meta' % i]]
        S, stride, iou_aware, mask = meta[0], meta[1], meta[2], meta[3:]
        o = torch.from_numpy(g['l%d_out' % i])
        c = dc.Case('g4_%d' % i, [o], [g['anchors'][mask].tolist()], [stride], 3, 80, 1.05, iou_aware, 0.4, True, im_size, 0.01, {})
        b, s = dc._decode(c, torch.float32)
        assert torch.equal(b, torch.from_numpy(g['l%d_boxes' % i])) and torch.equal(s, torch.from_numpy(g['l%d_scores' % i]))


def test_score_to_key_orders_like_the_scores():
    s = np.array([-1.0, -0.0, 0.0, 1e-45, 0.01, 1.0], dtype=np.float32)
    k = dc.score_to_key(s)
    assert (np.diff(k) > 0).all() and k[2] == 0x80000000
