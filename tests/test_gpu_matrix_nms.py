"""Matrix-NMS (csrc/decode_nms.hip + csrc/nms_select.h) on the cases of tests/matrix_nms_cases.py (whose own conditions
tests/test_matrix_nms_cases.py checks on the CPU), through ops.matrix_nms, against oracle.ppyolo_oracle.matrix_nms.

Every run gets a workspace filled with POISON, candidate buffers with a guard row behind the last image and sentinel-filled
outputs with a guard row; the guards are compared afterwards.  A case with `meta['route']` proves the route it took from the
NmsBig header of the workspace (ccount, bad), so its assertion fails if another route is taken:
  untouched    cand_cap <= 8192: sample / collect are not launched, the header keeps the poison
  cached       a list of at most 8192 entries: ccount == -1
  compact      sample + collect, the select runs on the compact list: nms_top_k <= ccount <= 32768, bad == 0
  compact_all  the same with every entry collected: ccount == the list's length == 32768
  too_long     ccount == the list's length == 32769 > 32768: the original list is walked
  overflow     one collect workgroup met more than 4096 survivors: bad == 1, the original list is walked

Linear kernel: rows, counts and keep indices are bit for bit the float32 oracle's, every padding row and keep index is -1.
Gaussian kernel (expf): the kept set equals the float32 oracle's (no exclusions: the builders keep every float64 score 1e-5 x
the largest away from post_threshold and from the cut), labels and boxes are exact, each score's error against float64 is at
most RATIO_BOUND = 4 x the float32 oracle's own on the same case (floor 1e-7 x the largest score), the output is non-increasing in
the kernel's own scores and never contradicts the float64 order by more than twice that bound.  Measured ratios:
profiles/matrix_nms_parity.txt.
"""
import numpy as np
import pytest
import torch

import matrix_nms_cases as mc
from test_gpu_ops import _nms_big_header

pytestmark = pytest.mark.gpu

POISON = -77                 # int32 fill of a workspace before a run
SENT = -5.0                  # outputs before a run
GUARD = -9                   # candidate rows behind the last image


class Run(object):
    pass


def _inputs(case):
    """Device inputs with a guard image behind the last one: boxes [N, M, 4], cand_key / cand_idx [N + 1, cap], cand_count."""
    from ppyolo_hip import ops
    N, cap = case.N, case.cand_cap
    r = Run()
    r.boxes = case.boxes.cuda()
    r.ck = torch.full((N + 1, cap), GUARD, dtype=torch.int32).cuda()
    r.ci = torch.full((N + 1, cap), GUARD, dtype=torch.int32).cuda()
    r.cc = torch.zeros(N + 1, dtype=torch.int32).cuda()
    if case.lists is None:
        ops.nms_candidates(case.scores.cuda(), case.thr, r.ck[:N], r.ci[:N], r.cc[:N])
    else:
        ck, ci = torch.full((N + 1, cap), GUARD, dtype=torch.int32), torch.full((N + 1, cap), GUARD, dtype=torch.int32)
        for n, (key, idx) in enumerate(case.lists):
            ck[n, :len(key)] = torch.from_numpy(key)
            ci[n, :len(idx)] = torch.from_numpy(idx)
        r.ck, r.ci = ck.cuda(), ci.cuda()
        r.cc = torch.tensor(list(case.counts) + [0], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    assert r.cc[:N].tolist() == ([int(c) for c in case.counts] if case.lists is not None else [case.used(n) for n in range(N)])
    return r


def _poisoned_ws(N):
    from ppyolo_hip import ops
    ws = ops.matrix_nms_workspace(N, 'cuda')
    ws.view(torch.int32).fill_(POISON)
    return ws


def _run(case, ws=None, inputs=None):
    """One ops.matrix_nms call -> Run with dets [N, keep_k, 6], cnt [N], keep [N, keep_k] on the host and the header (ccount,
    bad) per image.  ws: a workspace to reuse as it is (at least N images), None = a fresh poisoned one."""
    from ppyolo_hip import ops
    N, K = case.N, case.keep_k
    r = inputs or _inputs(case)
    ws = _poisoned_ws(N) if ws is None else ws
    dets = torch.full((N + 1, K, 6), SENT).cuda()
    cnt = torch.full((N + 1,), int(SENT), dtype=torch.int32).cuda()
    keep = torch.full((N + 1, K), int(SENT), dtype=torch.int32).cuda()
    before = (r.ck.clone(), r.ci.clone(), r.cc.clone())
    ops.matrix_nms(r.boxes, case.C, r.ck[:N], r.ci[:N], r.cc[:N], case.post, case.top_k, case.keep_k, case.gauss, case.sigma,
                   dets[:N], cnt[:N], keep[:N], ws=ws)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (r.ck, r.ci, r.cc))), 'the candidate lists are inputs'
    assert torch.all(dets[N] == SENT) and int(cnt[N]) == int(SENT) and torch.all(keep[N] == int(SENT)), 'output guard row'
    out = Run()
    out.dets, out.cnt, out.keep = dets[:N].cpu(), cnt[:N].cpu(), keep[:N].cpu()
    out.ccount, out.bad = _nms_big_header(ws, N)
    return out


def _same(a, b):
    return (np.array_equal(a.dets.numpy().view(np.int32), b.dets.numpy().view(np.int32)) and torch.equal(a.cnt, b.cnt)
            and torch.equal(a.keep, b.keep))


def _check_route(case, out):
    for n, route in enumerate(case.meta.get('route', [])):
        cc, bad, used = out.ccount[n], out.bad[n], case.used(n)
        what = '%s image %d: ccount %d, bad %d, %d entries' % (case.name, n, cc, bad, used)
        if route == 'untouched':
            assert case.cand_cap <= mc.CCAP and cc == POISON and bad == POISON, what
        elif route == 'cached':
            assert used <= mc.CCAP and cc == -1 and bad == 0, what
        elif route == 'compact':
            assert used > mc.CCAP and bad == 0 and case.top_k <= cc <= mc.NMS_CCAP2 and cc <= used, what
        elif route == 'compact_all':
            assert bad == 0 and cc == used == mc.NMS_CCAP2, what
        elif route == 'too_long':
            assert bad == 0 and cc == used == mc.NMS_CCAP2 + 1, what
        else:
            assert route == 'overflow' and bad == 1 and cc == mc.OVERFLOW_TIES > mc.NMS_CL, what


def _check_padding(case, out, n, k):
    assert torch.all(out.dets[n, k:] == -1) and torch.all(out.keep[n, k:] == -1), '%s image %d: padding' % (case.name, n)


def _check_linear(case, out, images=None):
    """Bit for bit the float32 oracle (image n of `case` is image images[n] of the oracle's case `case.meta['source']`)."""
    ref = mc.oracle(case.meta.get('source', case.name))
    for n in range(case.N):
        rows, keep = ref[n if images is None else images[n]]
        k = int(out.cnt[n])
        assert k == rows.shape[0], '%s image %d: %d rows, the oracle has %d' % (case.name, n, k, rows.shape[0])
        assert np.array_equal(out.dets[n, :k].numpy().view(np.int32), rows.numpy().view(np.int32)), (case.name, n)
        assert np.array_equal(out.keep[n, :k].numpy().astype(np.int64), keep), (case.name, n)
        _check_padding(case, out, n, k)


def _check_gauss(case, out, images=None):
    """-> (kernel error, float32 oracle's error, floor) of the case; asserts everything but the ratio."""
    src = case.meta.get('source', case.name)
    r32, r64 = mc.oracle(src), mc.oracle(src, torch.float64)
    per = []
    for n in range(case.N):
        m = n if images is None else images[n]
        rows, keep = r32[m]
        k = int(out.cnt[n])
        got_keep = out.keep[n, :k].numpy().astype(np.int64)
        assert k == rows.shape[0] and set(got_keep.tolist()) == set(keep.tolist()) and len(set(got_keep.tolist())) == k, \
            '%s image %d: kept set differs from the float32 oracle (%d rows against %d)' % (case.name, n, k, rows.shape[0])
        _check_padding(case, out, n, k)
        by_idx = dict((int(f), rows[i]) for i, f in enumerate(keep.tolist()))
        for i, f in enumerate(got_keep.tolist()):                  # labels and boxes are copies: exact
            want = by_idx[f]
            assert out.dets[n, i, 0] == want[0] and torch.equal(out.dets[n, i, 2:], want[2:]), (case.name, n, i)
        per.append(mc.score_errors(src, m, got_keep, out.dets[n, :k, 1].numpy()))
    err, e32, floor = [max(p[i] for p in per) for i in range(3)]
    bound = mc.bound_of(e32, floor)
    for n in range(case.N):
        k = int(out.cnt[n])
        own = out.dets[n, :k, 1]
        assert bool((own[:-1] >= own[1:]).all()), '%s image %d: not sorted by its own scores' % (case.name, n)
        rows64, keep64 = r64[n if images is None else images[n]]
        s64 = dict(zip(keep64.tolist(), rows64[:, 1].tolist()))
        seq = np.array([s64[f] for f in out.keep[n, :k].tolist()])
        if k > 1:                                                  # no later row is above an earlier one by more than 2 x bound
            later = np.maximum.accumulate(seq[::-1])[::-1]
            assert np.all(seq[:-1] >= later[1:] - 2 * bound), '%s image %d: order against float64' % (case.name, n)
    return err, e32, floor


def _judge(case, out, images=None):
    if not case.gauss:
        _check_linear(case, out, images)
        return
    err, e32, floor = _check_gauss(case, out, images)
    ratio = err / max(e32, floor) if max(e32, floor) > 0 else 0.0
    print('NMS-CASES %s: scores error vs float64 %.3e, float32 oracle %.3e, floor %.3e, ratio %.2f'
          % (case.name, err, e32, floor, ratio))
    assert err <= mc.bound_of(e32, floor), '%s: ratio %.2f above %g' % (case.name, ratio, mc.RATIO_BOUND)


SINGLE = [n for n in mc.names() if not n.startswith(('order_', 'batch_'))]


@pytest.mark.parametrize('name', SINGLE)
def test_case_against_the_oracle(name):
    case = mc.get(name)
    out = _run(case)
    _check_route(case, out)
    _judge(case, out)
    if name == 'post_equal_below':
        keep = out.keep[0, :int(out.cnt[0])].tolist()
        assert case.meta['equal'] in keep and case.meta['below'] not in keep
    if name == 'post_above_all':
        assert int(out.cnt[0]) == 0 and torch.all(out.dets == -1)
    if name in mc.INDEX_SHAPES:
        assert out.keep[0, :2].tolist() == [case.meta['first'], case.meta['last']]


@pytest.mark.parametrize('gauss', [False, True], ids=['linear', 'gauss'])
def test_batch_and_workspace_reuse(gauss):
    """Five unlike images in one call (a NaN-poisoned image leaves its neighbours alone), then N = 1 and N = 16 on the SAME
    workspace tensor, whose per-image sections move with N: the results equal those of a fresh workspace and the oracle."""
    from ppyolo_hip import ops
    base = mc.get('batch_gauss' if gauss else 'batch_linear')
    x16 = [i % 5 for i in range(16)]
    plans = [(base, list(range(5))), (mc.take(base, [3], base.name + '_x1'), [3]), (mc.take(base, x16, base.name + '_x16'), x16),
             (mc.take(base, [4, 1], base.name + '_x2'), [4, 1])]
    ws = ops.matrix_nms_workspace(16, 'cuda')
    ws.view(torch.int32).fill_(POISON)
    for case, images in plans:
        inputs = _inputs(case)
        reused, fresh = _run(case, ws=ws, inputs=inputs), _run(case, inputs=inputs)
        assert _same(reused, fresh), '%s: a reused workspace changes the result' % case.name
        _check_route(case, reused)
        _check_route(case, fresh)
        _judge(case, reused, images)
        for n, m in enumerate(images):
            if m in base.meta['nan_images'] or base.meta['kinds'][m] == 'empty':
                assert int(reused.cnt[n]) == 0 and torch.all(reused.dets[n] == -1) and torch.all(reused.keep[n] == -1)


@pytest.mark.parametrize('family', mc.ORDER_FAMILIES)
def test_list_order_is_free(family):
    """The candidate list is an unordered set: ascending index, descending score and a shuffle give the same bits."""
    outs = []
    for order in mc.ORDERS:
        case = mc.get('order_%s_%s' % (family, order))
        out = _run(case)
        _check_route(case, out)
        _check_linear(case, out)
        outs.append(out)
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])


def test_refusals_write_nothing():
    """nms_top_k outside 1 .. 1024 (the reference's `<= 0` = "no limit" is refused, not clamped), keep_top_k outside 1 ..
    nms_top_k and a short workspace raise and leave the outputs alone; model.matrix_nms.matrix_nms passes them through."""
    from model.matrix_nms import matrix_nms
    from ppyolo_hip import ops
    from ppyolo_hip._lib import PPYoloHipError
    case = mc.get('topk_63_63_many')
    r = _inputs(case)
    N = case.N
    ws = _poisoned_ws(N)
    bad = [(0, 1, ws), (-1, 1, ws), (mc.KMAX + 1, 100, ws), (100, 0, ws), (100, 101, ws), (1, 2, ws),
           (100, 50, ws[:ws.numel() - 1])]
    for topk, keepk, w in bad:
        rows = max(keepk, 1)
        dets = torch.full((N, rows, 6), SENT).cuda()
        cnt = torch.full((N,), int(SENT), dtype=torch.int32).cuda()
        keep = torch.full((N, rows), int(SENT), dtype=torch.int32).cuda()
        with pytest.raises(PPYoloHipError):
            ops.matrix_nms(r.boxes, case.C, r.ck[:N], r.ci[:N], r.cc[:N], case.post, topk, keepk, False, 2.0, dets, cnt, keep, ws=w)
        torch.cuda.synchronize()
        assert torch.all(dets == SENT) and torch.all(cnt == int(SENT)) and torch.all(keep == int(SENT)), (topk, keepk)
        assert torch.all(ws.view(torch.int32) == POISON), 'a refused call touched the workspace'
    for topk, keepk in [(0, 1), (-1, 1), (mc.KMAX + 1, 100), (100, 0), (100, 101)]:
        with pytest.raises(PPYoloHipError):
            matrix_nms(r.boxes[0], case.scores[0].cuda(), case.thr, case.post, topk, keepk)
    # and the accepted neighbour of each limit runs
    pred = matrix_nms(r.boxes[0], case.scores[0].cuda(), case.thr, case.post, mc.KMAX, mc.KMAX)
    rows, _ = mc.run_oracle(mc.Case('limit', case.boxes, case.scores, (case.thr, case.post, mc.KMAX, mc.KMAX, False, 2.0)), 0,
                            torch.float32)
    assert torch.equal(pred.cpu(), rows)
