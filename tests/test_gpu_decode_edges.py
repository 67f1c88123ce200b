"""The YOLO decode kernels (csrc/decode_nms.hip) on the cases of tests/decode_cases.py (whose own conditions
tests/test_decode_cases.py checks on the CPU): every head layout the entry points accept, the threshold ladder, the IoU-aware
clamps, box extremes and the thresholds 0, -0.5 and 1, against oracle.ppyolo_oracle in float32 and float64.

Every case runs through ops.yolo_decode with and without `scores_dense` (the staged kernel; without it the logit-domain
candidate bound is in force) and through ops.yolo_decode_levels (the streaming kernel where the layout allows it; the (3, 80)
cases once more with the staged kernel forced), on five row layouts in turn: head_ld == nch; nch rounded up to 4 with NaN
pads; the same at channel offset 4 of a wider buffer; head_ld = nch + 1; a base pointer one float past a 16-byte boundary
(the last two take the scalar loader, except that nch + 1 = 256 of the plain (3, 80) layout is a padded row again).  Boxes and
candidate buffers are over-allocated and sentinel-filled, the input is compared bit for bit afterwards.

Exact: list-only candidates == candidates of the dense call (this pins the bound), all runs and layouts give the same box
bits and the same (index, key) sets, key == score_to_key(dense score), indices unique, cand_count == #(dense > thr), the
non-finite and signed-zero patterns of the float32 oracle.  Versus float64: the kernel's error is at most RATIO_BOUND = 4 x
the float32 oracle's own (floor 1e-7), per box relative to max(1, |ref|), per score relative to the score; the candidate set
is {score64 > thr} outside the band of decode_cases.band (the thr_* cases: the float32 rule, no band).  Measured ratios:
profiles/decode_parity.txt.
"""
import numpy as np
import pytest
import torch

import decode_cases as dc
from oracle import ppyolo_oracle as orc

pytestmark = pytest.mark.gpu

SENT_BOX = 777.0
SENT_CAND = -7                # as a key: the bits of a NaN score, never a candidate; as an index: negative
GUARD_ROWS = 5
ROW_LAYOUTS = ['packed', 'padded', 'offset4', 'plus1', 'misaligned']
NAN = float('nan')


def _rows(o, layout):
    """NCHW head output -> (the whole device buffer, a View of its channels) in one of ROW_LAYOUTS."""
    from ppyolo_hip import ops
    N, nch, S, _ = o.shape
    x = o.permute(0, 2, 3, 1)
    up4 = (nch + 3) // 4 * 4
    if layout == 'misaligned':
        ld = up4 if up4 != nch else nch + 4
        flat = torch.full((N * S * S * ld + 4,), NAN)
        t = flat[1:1 + N * S * S * ld].view(N, S, S, ld)
        t[..., :nch] = x
        flat = flat.cuda()
        t = flat[1:1 + N * S * S * ld].view(N, S, S, ld)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return flat, ops.View(t, 0, nch)
    ld, coff = {'packed': (nch, 0), 'padded': (up4, 0), 'offset4': (up4 + 8, 4), 'plus1': (nch + 1, 0)}[layout]
    t = torch.full((N, S, S, ld), NAN)
    t[..., coff:coff + nch] = x
    t = t.cuda()
    return t, ops.View(t, coff, nch)


class Run(object):
    pass


def _run(case, views, mode, dense=False, cap=None):
    """One decode of all levels.  mode: 'single' (ops.yolo_decode per level), 'levels' (ops.yolo_decode_levels), 'levels_staged'
    (the same with the staged kernel forced).  Checks the guards; -> Run with boxes [N, M, 4], dense [N, M, C] or None (host),
    count [N], and per image the stored (index, key) pairs sorted by index."""
    from ppyolo_hip import ops
    from ppyolo_hip._lib import lib
    N, M, C = case.N, case.M, case.C
    Mt = M + GUARD_ROWS
    cap = M * C + 3 if cap is None else cap
    boxes = torch.full((N + 1, Mt, 4), SENT_BOX).cuda()
    ck = torch.full((N + 1, cap), SENT_CAND, dtype=torch.int32).cuda()
    ci = torch.full((N + 1, cap), SENT_CAND, dtype=torch.int32).cuda()
    cc = torch.zeros(N + 1, dtype=torch.int32).cuda()
    sd = torch.full((N + 1, Mt, C), SENT_BOX).cuda() if dense else None
    im = case.im_size.cuda()
    args = (case.C, case.scale_x_y, case.iou_aware, case.factor, case.clip, im, boxes[:N])
    if mode == 'single':
        off = 0
        for v, anc, st in zip(views, case.anchors, case.strides):
            ops.yolo_decode(v, anc, st, *args, off, case.thr, ck[:N], ci[:N], cc[:N], sd[:N] if dense else None)
            off += v.H * v.W * case.A
    else:
        assert not dense
        lib().ppy_debug_decode_mode(1 if mode == 'levels_staged' else 0, -1, 0)
        try:
            ops.yolo_decode_levels(views, case.anchors, case.strides, *args, case.thr, ck[:N], ci[:N], cc[:N])
            torch.cuda.synchronize()
        finally:
            lib().ppy_debug_decode_mode(-1, -1, 0)
    torch.cuda.synchronize()
    r = Run()
    r.dev = (boxes[:N], ck[:N], ci[:N], cc[:N])
    b, k, i, c = boxes.cpu(), ck.cpu(), ci.cpu(), cc.cpu()
    assert (b[N] == SENT_BOX).all() and (b[:N, M:] == SENT_BOX).all(), 'boxes written outside [box_offset, box_offset + S*S*A)'
    assert c[N] == 0 and (k[N] == SENT_CAND).all() and (i[N] == SENT_CAND).all(), 'candidate buffers written past the batch'
    r.boxes, r.count, r.pairs, r.dense = b[:N, :M], c[:N].long(), [], None
    for n in range(N):
        st = min(int(c[n]), cap)
        assert (k[n, st:] == SENT_CAND).all() and (i[n, st:] == SENT_CAND).all(), 'candidate list written past min(count, cap)'
        p = torch.stack([i[n, :st].long(), k[n, :st].long() & 0xffffffff], 1)
        r.pairs.append(p[torch.argsort(p[:, 0])])
    if dense:
        s = sd.cpu()
        assert (s[N] == SENT_BOX).all() and (s[:N, M:] == SENT_BOX).all(), 'dense scores written outside the level\'s rows'
        r.dense = s[:N, :M]
    return r


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_list(case, r, dense):
    """The candidate list of `r` against the dense scores of the same kernel: count, uniqueness, set, keys."""
    flat = dense.reshape(case.N, -1)
    assert torch.equal(r.count, (flat > case.thr).sum(1)), (case.name, r.count, (flat > case.thr).sum(1))
    for n in range(case.N):
        idx = r.pairs[n][:, 0]
        assert idx.numel() == int(r.count[n])
        assert torch.unique(idx).numel() == idx.numel(), 'a candidate index appears twice'
        assert torch.equal(idx, torch.nonzero(flat[n] > case.thr).flatten()), (case.name, n)
        keys = torch.from_numpy(dc.score_to_key(flat[n][idx].numpy()))
        assert torch.equal(r.pairs[n][:, 1], keys), 'a key is not score_to_key of the dense score at its index'


def _same(case, r, ref, what):
    assert torch.equal(_bits(r.boxes), _bits(ref.boxes)), '%s %s: boxes differ' % (case.name, what)
    assert torch.equal(r.count, ref.count), '%s %s: cand_count %s vs %s' % (case.name, what, r.count.tolist(), ref.count.tolist())
    for n in range(case.N):
        assert torch.equal(r.pairs[n], ref.pairs[n]), '%s %s: candidate (index, key) sets differ in image %d' % (case.name, what, n)


def _small_cap(case, views, mode, ref):
    cap = max(1, int(ref.count.max()) // 3)
    r = _run(case, views, mode, cap=cap)
    assert torch.equal(r.count, ref.count), 'cand_count must hold the true total when the list overflows'
    for n in range(case.N):
        assert r.pairs[n].shape[0] == min(int(ref.count[n]), cap)
        true = set(map(tuple, ref.pairs[n].tolist()))
        assert set(map(tuple, r.pairs[n].tolist())) <= true
    assert torch.equal(_bits(r.boxes), _bits(ref.boxes))


def decode_everywhere(name):
    """All runs on all row layouts, compared with one another bit for bit -> the dense run of the first layout."""
    case = dc.get(name)
    coco = (case.A, case.C) == (3, 80)
    ref = None
    for layout in ROW_LAYOUTS:
        bufs, views = zip(*[_rows(o, layout) for o in case.outs])
        before = [b.clone() for b in bufs]
        full = _run(case, views, 'single', dense=True)
        _check_list(case, full, full.dense)
        _same(case, _run(case, views, 'single'), full, layout + ' list-only vs dense call')
        _same(case, _run(case, views, 'levels'), full, layout + ' yolo_decode_levels vs dense call')
        if coco:
            _same(case, _run(case, views, 'levels_staged'), full, layout + ' staged yolo_decode_levels vs dense call')
        if layout == 'packed':
            ref = full
            _small_cap(case, views, 'single', ref)
        else:
            _same(case, full, ref, layout + ' vs packed')
            assert torch.equal(_bits(full.dense), _bits(ref.dense)), '%s %s: dense scores differ' % (name, layout)
        if layout == 'padded':
            _small_cap(case, views, 'levels', ref)
            if coco:
                _small_cap(case, views, 'levels_staged', ref)
        for b, b0 in zip(bufs, before):
            assert torch.equal(_bits(b), _bits(b0)), 'the input is only read'
    return case, ref


def _pattern(t):
    nan = torch.isnan(t)
    return nan, torch.isinf(t), torch.signbit(t) & ~nan


def check_against_oracle(name, case, ref):
    (b32, s32), (b64, s64) = dc.oracle(name, torch.float32), dc.oracle(name, torch.float64)
    for what, got, want in (('boxes', ref.boxes, b32), ('scores', ref.dense, s32)):
        for kind, g, w in zip(('isnan', 'isinf', 'signbit'), _pattern(got), _pattern(want)):
            assert torch.equal(g, w), '%s: %s pattern of the %s differs at %s' % (name, kind, what, torch.nonzero(g != w)[:5].tolist())
    under = torch.isfinite(s64) & ~dc.normal_scores(name)          # below the normal float32 range: no relative error there
    assert ((ref.dense[under] >= 0) & (ref.dense[under] <= 2 * dc.FLT_MIN)).all()
    ratios = {}
    for what, e_hip, e_ref in (('boxes', dc.rel_box_error(ref.boxes, name), dc.rel_box_error(b32, name)),
                               ('scores', dc.rel_score_error(ref.dense, name), dc.e32(name))):
        ratios[what] = e_hip / max(e_ref, dc.ERR_FLOOR)
        print('DECODE-EDGES %s: %s error vs float64 %.3e, float32 oracle %.3e, ratio %.2f' % (name, what, e_hip, e_ref, ratios[what]))
    cand = torch.zeros(case.N, case.M * case.C, dtype=torch.bool)
    for n in range(case.N):
        cand[n, ref.pairs[n][:, 0]] = True
    cand = cand.reshape(s64.shape)
    if name in dc.NO_BAND:
        assert torch.equal(cand, s32 > case.thr), '%s: candidates differ from the reference\'s score > thr at %s' % (
            name, torch.nonzero(cand != (s32 > case.thr))[:5].tolist())
    else:
        bd = dc.band(name)
        wrong = (cand != (s64 > case.thr)) & ~bd
        print('DECODE-EDGES %s: %d pairs in the band, %d of them decided against float64' % (name, int(bd.sum()), int((cand != (s64 > case.thr)).sum())))
        assert not wrong.any(), '%s: candidates differ from score64 > thr outside the band at %s' % (name, torch.nonzero(wrong)[:5].tolist())
    assert max(ratios.values()) <= dc.RATIO_BOUND, (name, ratios)


@pytest.mark.parametrize('name', dc.names())
def test_decode_case(name):
    case, ref = decode_everywhere(name)
    if name == dc.ALL_PASS:
        assert (ref.count > 0.99 * case.M * case.C).all()
    check_against_oracle(name, case, ref)


@pytest.mark.parametrize('name', dc.NMS_CASES)
def test_decode_through_matrix_nms(name):
    """ops.matrix_nms (hard kernel) on the decode's own list against oracle.matrix_nms on the kernel's boxes and dense scores:
    rows and keep indices equal, as tests/test_gpu_ops.py::test_matrix_nms_golden_bit_exact asserts them."""
    from ppyolo_hip import ops
    case = dc.get(name)
    views = [_rows(o, 'packed')[1] for o in case.outs]
    full = _run(case, views, 'single', dense=True)
    lst = _run(case, views, 'single')
    post, top_k, keep_k = 0.01, 100, 50
    N = case.N
    dets = torch.zeros(N, keep_k, 6).cuda()
    cnt = torch.zeros(N, dtype=torch.int32).cuda()
    keep = torch.zeros(N, keep_k, dtype=torch.int32).cuda()
    boxes, ck, ci, cc = lst.dev
    ops.matrix_nms(boxes, case.C, ck, ci, cc, post, top_k, keep_k, False, 2.0, dets, cnt, keep)
    torch.cuda.synchronize()
    dets, cnt, keep = dets.cpu(), cnt.cpu(), keep.cpu()
    for n in range(N):
        assert int(full.count[n]) > top_k                                   # the top-k selection is exercised
        want, f = orc.matrix_nms(full.boxes[n], full.dense[n], case.thr, post, top_k, keep_k, False, 2.0, return_index=True)
        k = int(cnt[n])
        assert k == want.shape[0] and want[0, 0] >= 0, (name, n, k, want.shape)
        assert torch.equal(dets[n, :k, 0], want[:, 0]) and torch.equal(dets[n, :k, 2:], want[:, 2:])
        assert torch.equal(dets[n, :k, 1], want[:, 1]), 'scores not bit-exact'
        assert np.array_equal(keep[n, :k].numpy().astype(np.int64), f)
        assert torch.all(keep[n, k:] == -1) and torch.all(dets[n, k:] == -1)


def test_refusals_write_nothing():
    """nch = 273 ((3, 85) with the IoU channels), nine anchors and a box_offset past M_total raise; no buffer is touched."""
    from ppyolo_hip import ops
    from ppyolo_hip._lib import PPYoloHipError
    S, N = 2, 1
    im = torch.tensor(dc.IM_SIZES[:N]).cuda()

    def attempt(A, C, iou_aware, off, levels=False):
        nch = A * (5 + C) + (A if iou_aware else 0)
        M = S * S * A
        head = ops.View(torch.zeros(N, S, S, nch).cuda())
        boxes = torch.full((N, M + 2, 4), SENT_BOX).cuda()
        ck = torch.full((N, M * C), SENT_CAND, dtype=torch.int32).cuda()
        ci, cc = ck.clone(), torch.zeros(N, dtype=torch.int32).cuda()
        anchors = [[10 + a, 13 + a] for a in range(A)]
        with pytest.raises(PPYoloHipError):
            if levels:
                ops.yolo_decode_levels([head], [anchors], [32], C, 1.05, iou_aware, 0.4, True, im, boxes, 0.01, ck, ci, cc)
            else:
                ops.yolo_decode(head, anchors, 32, C, 1.05, iou_aware, 0.4, True, im, boxes, off, 0.01, ck, ci, cc)
        torch.cuda.synchronize()
        assert (boxes == SENT_BOX).all() and (ck == SENT_CAND).all() and (ci == SENT_CAND).all() and (cc == 0).all()
    attempt(3, 85, True, 0)
    attempt(3, 85, True, 0, levels=True)
    attempt(9, 3, False, 0)
    attempt(9, 3, False, 0, levels=True)
    attempt(3, 80, True, 3)                      # box_offset + S*S*A = M_total + 1
    attempt(3, 80, True, S * S * 3 + 3)          # box_offset past M_total
