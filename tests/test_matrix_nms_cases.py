"""The builders of tests/matrix_nms_cases.py meet their own conditions, and the oracle equals the reference itself on every
tie-free case (tests/golden/g25_matrix_nms_cases.npz, written by tools/make_goldens.py --only g25).  No device."""
import numpy as np
import pytest
import torch

import matrix_nms_cases as mc
from oracle import ppyolo_oracle as orc


def test_key_is_order_preserving_and_matches_the_header():
    s = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 0.01, 0.25, 1.0, 7.0, np.inf], dtype=np.float32)
    k = mc.score_key(s).astype(np.int64)
    assert np.all(np.diff(k) > 0)
    bits = s.view(np.uint32).astype(np.int64)
    for b, key, v in zip(bits, k, s):
        expect = (b ^ 0x80000000) if not np.signbit(v) else (~b & 0xffffffff)
        assert key == expect
    assert np.array_equal(mc.key_score(mc.score_key(s)).view(np.uint32), s.view(np.uint32))
    # the int32 bit patterns of a list, its three orders, and the dense scores it stands for
    sc = torch.tensor([[0.5, 0.0], [0.02, 0.7], [0.7, 0.009]])
    for order, want in (('index', [0, 2, 3, 4]), ('score', [3, 4, 0, 2])):
        key, idx = mc.candidate_list(sc, mc.THR, order)
        assert key.dtype == np.int32 and idx.dtype == np.int32 and idx.tolist() == want
        assert np.array_equal(key.view(np.uint32), mc.score_key(sc.reshape(-1).numpy()[idx]))
        assert torch.equal(mc.dense_of(key, idx, 3, 2), torch.where(sc > mc.THR, sc, torch.zeros(())))
    key, idx = mc.candidate_list(sc, mc.THR, 'shuffle', seed=3)
    assert sorted(idx.tolist()) == [0, 2, 3, 4]


def test_every_case_is_well_formed():
    for name in mc.names():
        c = mc.get(name)
        assert c.boxes.shape == (c.N, c.M, 4) and c.scores.shape == (c.N, c.M, c.C)
        assert 1 <= c.keep_k <= c.top_k <= mc.KMAX and c.thr >= 0 and c.M * c.C < 2 ** 31
        if c.lists is not None:
            for n, (key, idx) in enumerate(c.lists):
                assert len(key) == len(idx) == c.used(n) <= c.cand_cap and c.counts[n] >= len(key)
                assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < c.M * c.C
                # the stored entries are exactly the dense candidates
                k2, i2 = mc.candidate_list(c.scores[n], c.thr, 'index')
                o = np.argsort(idx)
                assert np.array_equal(idx[o], i2) and np.array_equal(key[o], k2)
        else:
            assert all(c.used(n) <= c.cand_cap for n in range(c.N))
        if c.tie_free:
            for n in range(c.N):
                s = c.scores[n][c.scores[n] > c.thr]
                assert len(torch.unique(s)) == len(s), name
                rows, _ = mc.oracle(name)[n]
                assert len(torch.unique(rows[:, 1])) == rows.shape[0], name


@pytest.mark.parametrize('topk,keepk', mc.TOPK)
def test_topk_counts(topk, keepk):
    for kind, counts in (('edge', [topk - 1, topk, topk + 1]), ('many', [1200])):
        c = mc.get('topk_%d_%d_%s' % (topk, keepk, kind))
        assert (c.top_k, c.keep_k, c.M, c.C) == (topk, keepk, 300, 5)
        assert [c.used(n) for n in range(c.N)] == counts
        for n in range(c.N):
            rows, keep = mc.oracle(c.name)[n]
            assert len(keep) <= min(keepk, counts[n])
    # the rank sort's pad: 64 for K <= 64, 128 at 65, 1024 at 1024
    pad = lambda K: max(64, 1 << (K - 1).bit_length())
    assert [pad(K) for K in (1, 63, 64, 65, 500, 1024)] == [64, 64, 64, 128, 512, 1024]


def test_route_preconditions():
    c = mc.get('route_scalar_c81')
    assert c.cand_cap % 4 != 0 and (c.cand_cap * 4) % 16 != 0 and c.lists is None      # odd capacity: image 1 is misaligned
    assert all(c.used(n) > mc.CCAP for n in range(c.N))
    v = mc.get('route_vector_c80')
    assert v.cand_cap % 4 == 0 and all(v.used(n) > mc.CCAP for n in range(v.N))
    for topk in (1024, 100):
        a, b = mc.get('route_list_8192_k%d' % topk), mc.get('route_list_8193_k%d' % topk)
        assert a.used(0) == mc.CCAP and b.used(0) == mc.CCAP + 1 and a.cand_cap > mc.CCAP and a.top_k == b.top_k == topk
        assert a.meta['route'] == ['cached'] and b.meta['route'] == ['compact']
    for count, route in ((mc.NMS_CCAP2, 'compact_all'), (mc.NMS_CCAP2 + 1, 'too_long')):
        c = mc.get('route_ties_%d' % count)
        assert c.used(0) == count and c.meta['route'] == [route]
        assert len(np.unique(c.lists[0][0])) == 1                  # one value: count(key >= any sampled threshold) == length
        assert count // mc.NMS_CG + 4 < mc.NMS_CL                   # no collect workgroup overflows on the way
    c = mc.get('route_collect_overflow')
    key, idx = c.lists[0]
    lo, hi, per = c.meta['tie_slice']
    assert c.used(0) == 400000 and np.array_equal(idx, np.arange(400000)) and hi - lo == mc.OVERFLOW_TIES > mc.NMS_CL
    top = key.view(np.uint32).max()
    tied = np.nonzero(key.view(np.uint32) == top)[0]
    assert tied[0] == lo and tied[-1] == hi - 1 and len(tied) == hi - lo and lo // per == (hi - 1) // per      # one slice
    rest = np.delete(key.view(np.uint32), tied)
    assert len(np.unique(rest)) == len(rest) and rest.max() < top
    # strata of the sampler wholly inside the tie against the rank it aims at (4 x nms_top_k x 8192 / count, at least 16)
    S = mc.CCAP
    inside = sum(1 for i in range(S) if i * 400000 // S >= lo and (i + 1) * 400000 // S <= hi)
    assert inside >= 2 * max(16, -(-4 * c.top_k * S // 400000))
    for name, count, cap in (('route_count_7000_cap_5000', 7000, 5000), ('route_count_20000_cap_9000', 20000, 9000)):
        c = mc.get(name)
        assert c.counts == [count, count] and c.cand_cap == cap and all(len(k) == cap for k, _ in c.lists)
        assert (cap <= mc.CCAP) == (c.meta['route'][0] == 'untouched')


def test_gauss_margins_and_equal_kept_sets():
    names = mc.names('gauss_') + ['batch_gauss']
    assert {mc.get(n).sigma for n in names} == set(mc.SIGMAS)
    for name in names:
        c = mc.get(name)
        assert c.gauss and c.N >= 2
        for n, (dist, gap, top) in enumerate(mc.margins(name)):
            assert dist >= mc.MARGIN * top and gap >= mc.MARGIN * top, (name, n, dist, gap)
            _, k32 = mc.oracle(name)[n]
            _, k64 = mc.oracle(name, torch.float64)[n]
            assert set(k32.tolist()) == set(k64.tolist()), (name, n)
    assert all(mc.get('gauss_big_list').used(n) > mc.CCAP for n in range(2))
    # comp == 1: the lower-scored copy of a duplicated box has a column maximum of exactly 1
    c = mc.get('gauss_dup')
    for n in range(c.N):
        order = torch.argsort(c.scores[n].reshape(-1), descending=True)
        b, lab = c.boxes[n][order // c.C], order % c.C
        d = orc.pairwise_iou(b, b).triu(1) * (lab[:, None] == lab[None, :]).float().triu(1)
        assert int((d.max(0)[0] == 1.0).sum()) == c.C * len(mc.DUPS)
    # the zero-area pair: the sentinel in both precisions, the neighbour untouched
    c = mc.get('gauss_nan')
    assert len(mc.oracle(c.name)[0][1]) == 0 and len(mc.oracle(c.name, torch.float64)[0][1]) == 0
    assert len(mc.oracle(c.name)[1][1]) == c.keep_k


def test_post_cases():
    c = mc.get('post_equal_below')
    rows, keep = mc.oracle(c.name)[0]
    eq, below = c.meta['equal'], c.meta['below']
    assert eq in keep.tolist() and below not in keep.tolist()
    assert float(rows[keep.tolist().index(eq), 1]) == c.post == mc.POST_P
    assert np.float32(c.meta['below_score']) < np.float32(c.post)
    assert np.nextafter(np.float32(c.meta['below_score']), np.float32(1)) == np.float32(c.post)
    # the coefficient of both isolated boxes is exactly 1: with no post_threshold their scores come back unchanged
    allr, allk = orc.matrix_nms(c.boxes[0], c.scores[0], c.thr, float('-inf'), c.top_k, c.top_k, False, 2.0, return_index=True)
    got = dict(zip(allk.tolist(), allr[:, 1].tolist()))
    assert got[eq] == c.post and got[below] == c.meta['below_score']
    c = mc.get('post_zero_dups')
    rows, keep = mc.oracle(c.name)[0]
    zeros = rows[:, 1] == 0.0
    assert c.post == 0.0 and int(zeros.sum()) == c.meta['zeros'] and bool(zeros[-c.meta['zeros']:].all())
    assert len(keep) == c.used(0)                                  # nothing is NaN, everything is kept
    # the tied zeros come in first-sort order: descending original score
    orig = c.scores[0].reshape(-1)[torch.from_numpy(keep[-c.meta['zeros']:])]
    assert bool((orig[:-1] > orig[1:]).all())
    c = mc.get('post_above_all')
    assert c.post > float(c.scores.max()) and c.used(0) > 0 and len(mc.oracle(c.name)[0][1]) == 0


def test_index_cases():
    bits = lambda span: max(1, (span - 1).bit_length())
    assert {n: bits(M * C) for n, (M, C) in mc.INDEX_SHAPES.items()} == {
        'index_c1_4096': 12, 'index_c1_4097': 13, 'index_c3_4095': 12, 'index_c3_4098': 13, 'index_c4_4096': 12}
    assert {C for _, C in mc.INDEX_SHAPES.values()} == {1, 3, 4}
    for name in mc.INDEX_SHAPES:
        c = mc.get(name)
        s = c.scores[0].reshape(-1)
        assert c.meta['last'] == c.M * c.C - 1 and s[0] == s[-1] == s.max() and int((s == s.max()).sum()) == 2
        rows, keep = mc.oracle(name)[0]
        assert keep[:2].tolist() == [0, c.M * c.C - 1] and rows[0, 1] == rows[1, 1] == s.max()       # undecayed, flat 0 first


def test_batch_and_order_cases():
    for name in ('batch_linear', 'batch_gauss'):
        c = mc.get(name)
        assert c.N == 5 and c.meta['kinds'] == mc.BATCH_KINDS
        used = [c.used(n) for n in range(5)]
        assert used[0] == 0 and used[2] == 1 and used[3] > mc.CCAP and 0 < used[1] <= mc.CCAP and 0 < used[4] <= mc.CCAP
        got = [len(k) for _, k in mc.oracle(name)]
        assert got[0] == 0 and got[1] == 0 and got[2] == 1 and got[3] == c.keep_k and got[4] == c.keep_k
        sub = mc.take(c, [i % 5 for i in range(16)], name + '_x16')
        assert sub.N == 16 and torch.equal(sub.scores[7], c.scores[2]) and sub.meta['route'][8] == 'compact'
    assert torch.equal(mc.get('batch_linear').scores, mc.get('batch_gauss').scores)
    for fam in mc.ORDER_FAMILIES:
        cases = [mc.get('order_%s_%s' % (fam, o)) for o in mc.ORDERS]
        base = cases[0]
        assert np.all(np.diff(base.lists[0][1]) > 0)
        sk = cases[1].lists[0][0].view(np.uint32).astype(np.int64)
        assert np.all(np.diff(sk) <= 0)
        for c in cases[1:]:
            assert torch.equal(c.scores, base.scores) and torch.equal(c.boxes, base.boxes)
            assert not np.array_equal(c.lists[0][1], base.lists[0][1])
            assert sorted(c.lists[0][1].tolist()) == base.lists[0][1].tolist()
    assert mc.get('order_small_index').used(0) <= mc.CCAP < mc.get('order_large_index').used(0)
    assert not mc.get('order_ties_index').tie_free


def test_oracle_equals_the_reference_on_tie_free_cases(golden):
    g = golden('g25_matrix_nms_cases')
    names = mc.golden_names()
    assert [str(n) for n in g['names']] == names and len(names) >= 35
    for name in names:
        c = mc.get(name)
        assert np.array_equal(g[name + '.cfg'], np.array(c.cfg + (c.N, c.M, c.C, c.meta.get('seed', -1)), dtype=np.float64)), name
        for n in range(c.N):
            ref = g['%s.%d' % (name, n)]
            rows, _ = mc.oracle(name)[n]
            if ref[0, 0] < 0:
                assert rows.shape[0] == 0 and ref.shape == (1, 6), (name, n)
            else:
                assert np.array_equal(rows.numpy().view(np.int32), ref.view(np.int32)), (name, n)
