"""ppy_merge_views_f32 (csrc/merge_views.hip) against the numpy restatement tests/tile_merge_ref.py, bit for bit: dets, count, src
and the padding.  The cases are the restatement's own (tests/test_tile_merge_ref.py derives the hand cases' answers and checks that
every seeded case selects, suppresses and, where it says so, cuts)."""
import numpy as np
import pytest
import torch

import tile_merge_ref as R

pytestmark = pytest.mark.gpu


def gpu_run(c, ws=None, **kw):
    """The kernel on a case -> numpy (dets, count, src)."""
    from ppyolo_hip import ops
    p = dict(c['kw'])
    p.update(kw)
    dets, count = torch.from_numpy(c['dets']).cuda(), torch.from_numpy(c['count']).cuda()
    tab = ops.merge_views_table(c['views'])
    n, k = c['n'], p['keep_top_k']
    out = (torch.full((n, k, 6), 7.0, dtype=torch.float32, device='cuda'), torch.full((n,), 7, dtype=torch.int32, device='cuda'),
           torch.full((n, k, 2), 7, dtype=torch.int32, device='cuda'))
    ops.merge_views(dets, count, tab, torch.from_numpy(tab).cuda(), n, p['metric'], p['thresh'], p['score_thresh'], p['class_agnostic'],
                    k, *out, ws=ws)
    return tuple(t.cpu().numpy() for t in out)


def same(got, want, what=''):
    for g, w, name in zip(got, want, ('dets', 'count', 'src')):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g.view(np.int32) != w.view(np.int32))[:4])


@pytest.mark.parametrize('name', sorted(R.hand_cases()))
def test_hand_cases(name):
    c = R.hand_cases()[name]
    same(gpu_run(c), R.run(c), name)


@pytest.mark.parametrize('i', range(len(R.SPREAD)))
def test_clustered_recipe_spread_over_views(i):
    V, K = R.SPREAD[i]
    c = R.spread_case(R.SEEDS[i % len(R.SEEDS)], V, K)
    for metric, agnostic in R.MODES:
        sel = [R.merge_image(c['dets'], c['count'], c['views'], 0, metric, 0.5, 0.3, agnostic)]      # once; the cuts are prefixes
        assert len(sel[0][0]) >= 1
        for keep in R.KEEPS:
            same(gpu_run(c, metric=metric, class_agnostic=agnostic, keep_top_k=keep), R.padded(c['dets'], sel, keep), (V, K, metric, agnostic, keep))


@pytest.fixture(scope='module')
def full_case():
    c = R.uniform_case(*R.BOUNDARIES[-1])
    return c, R.run(c)


@pytest.mark.parametrize('rows,V,K', R.BOUNDARIES[:-1])
def test_rows_at_the_stage_boundaries(rows, V, K):
    """A 64-candidate chunk of the scan +-1 and the counting sort's size +-1 (beyond it the bitonic network orders)."""
    from ppyolo_hip import _lib
    assert rows in (_lib.MERGE_CHUNK - 1, _lib.MERGE_CHUNK, _lib.MERGE_CHUNK + 1, _lib.MERGE_RANK_MAX - 1, _lib.MERGE_RANK_MAX,
                    _lib.MERGE_RANK_MAX + 1)
    c = R.uniform_case(rows, V, K)
    same(gpu_run(c), R.run(c), rows)
    same(gpu_run(c, metric='ios', class_agnostic=False, thresh=0.5), R.run(c, metric='ios', class_agnostic=False, thresh=0.5), rows)


def test_the_most_rows_an_image_may_have(full_case):
    from ppyolo_hip import _lib
    c, want = full_case
    assert c['dets'].shape[0] * c['dets'].shape[1] == _lib.MERGE_MAX_ROWS and want[1][0] == 1024
    same(gpu_run(c), want)


def test_one_row_more_is_refused():
    from ppyolo_hip._lib import PPYoloHipError
    rows, V, K = R.TOO_MANY
    c = dict(dets=np.zeros((V, K, 6), np.float32), count=np.zeros((V,), np.int32), views=np.zeros((V, 3), np.int32), n=1,
             kw=dict(metric='ios', thresh=0.5, score_thresh=0.0, class_agnostic=False, keep_top_k=10))
    with pytest.raises(PPYoloHipError, match='3 views x 2731 rows = 8193 rows, at most 8192'):
        gpu_run(c)


def test_batch_with_an_empty_a_padded_and_a_full_image(full_case):
    c = R.batch_case()
    got = gpu_run(c)
    same(got, R.run(c))
    assert got[1].tolist() == [0, 0, 1024]
    assert got[0][2].tobytes() == full_case[1][0][0].tobytes()          # image 2 is the full case, whatever surrounds it


def test_views_of_two_images_interleaved():
    c = R.interleaved_case()
    want = R.run(c)
    assert want[1].min() >= 1
    same(gpu_run(c), want)
    same(gpu_run(c, metric='iou', class_agnostic=True, keep_top_k=7), R.run(c, metric='iou', class_agnostic=True, keep_top_k=7))


def test_small_call_after_a_large_one_on_the_same_workspace(full_case):
    from ppyolo_hip import ops
    big, want_big = full_case
    ws = ops.merge_views_workspace(1, 64, 128, 'cuda')
    assert ws.numel() == 32 * 8192
    same(gpu_run(big, ws=ws), want_big)
    for name in ('halves_ios', 'padding_view', 'left_out'):
        c = R.hand_cases()[name]
        same(gpu_run(c, ws=ws), R.run(c), name)
    small = R.spread_case(2, 5, 7)
    same(gpu_run(small, ws=ws), R.run(small))


def test_two_runs_give_the_same_bytes(full_case):
    for c in (full_case[0], R.spread_case(3, 41, 100), R.interleaved_case()):
        a, b = gpu_run(c), gpu_run(c)
        same(a, b)


def test_no_host_synchronisation_and_graph_capture():
    """One launch, capturable: the replayed graph writes what the eager call wrote."""
    from ppyolo_hip import ops
    c = R.spread_case(0, 41, 100)
    p = c['kw']
    dets, count = torch.from_numpy(c['dets']).cuda(), torch.from_numpy(c['count']).cuda()
    tab = ops.merge_views_table(c['views'])
    d_tab = torch.from_numpy(tab).cuda()
    ws = ops.merge_views_workspace(1, 41, 100, 'cuda')
    out = (torch.empty((1, 40, 6), dtype=torch.float32, device='cuda'), torch.empty((1,), dtype=torch.int32, device='cuda'),
           torch.empty((1, 40, 2), dtype=torch.int32, device='cuda'))

    def call():
        ops.merge_views(dets, count, tab, d_tab, 1, p['metric'], p['thresh'], p['score_thresh'], False, 40, *out, ws=ws)
    call()
    torch.cuda.synchronize()
    eager = [t.clone() for t in out]
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call()
    for t in out:
        t.fill_(3)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    same(tuple(t.cpu().numpy() for t in out), R.run(c, keep_top_k=40))


@pytest.mark.parametrize('kw,word', [(dict(keep_top_k=0), 'keep_top_k = 0, supported: 1..1024'), (dict(keep_top_k=1025), 'keep_top_k = 1025'),
                                     (dict(thresh=float('nan')), 'thresh is NaN'), (dict(score_thresh=float('nan')), 'score_thresh is NaN'),
                                     (dict(metric='giou'), "unknown metric 'giou'")])
def test_refusals_by_name(kw, word):
    from ppyolo_hip._lib import PPYoloHipError
    c = R.hand_cases()['halves_ios']
    if 'keep_top_k' in kw:          # (the outputs cannot have the refused shape: any will do, the call ends before it reads them)
        from ppyolo_hip import ops
        dets, count = torch.from_numpy(c['dets']).cuda(), torch.from_numpy(c['count']).cuda()
        tab = ops.merge_views_table(c['views'])
        out = (torch.empty((1, 1, 6), device='cuda'), torch.empty((1,), dtype=torch.int32, device='cuda'),
               torch.empty((1, 1, 2), dtype=torch.int32, device='cuda'))
        with pytest.raises(PPYoloHipError, match=word):
            ops.merge_views(dets, count, tab, torch.from_numpy(tab).cuda(), 1, 'ios', 0.5, 0.0, False, kw['keep_top_k'], *out)
        return
    with pytest.raises(PPYoloHipError, match=word):
        gpu_run(c, **kw)


def test_refusals_of_the_table_and_the_workspace():
    from ppyolo_hip import ops
    from ppyolo_hip._lib import PPYoloHipError
    c = R.hand_cases()['halves_ios']
    bad = dict(c, views=c['views'].copy())
    bad['views'][1, 0] = 1                                   # image 1 of n = 1
    with pytest.raises(PPYoloHipError, match='code -1'):
        gpu_run(bad)
    with pytest.raises(PPYoloHipError, match='workspace'):
        gpu_run(c, ws=torch.empty(16, dtype=torch.uint8, device='cuda'))
    zero_k = dict(c, dets=np.zeros((3, 0, 6), np.float32))
    with pytest.raises(PPYoloHipError, match='K = 0 rows per view'):
        gpu_run(zero_k, ws=torch.empty(64, dtype=torch.uint8, device='cuda'))
    assert gpu_run(c)[1].tolist() == [1]                     # and it still works
