"""ppy_fuse_views_f32 (csrc/fuse_views.hip) against the numpy restatement tests/fuse_views_ref.py, bit for bit: dets, count, src,
members and the padding.  The cases are the restatement's own (tests/test_fuse_views_ref.py derives the hand cases' answers and
checks on the CPU that every seeded case forms what it names); each test here asserts the same from the stats again."""
import numpy as np
import pytest
import torch

import fuse_views_ref as R

pytestmark = pytest.mark.gpu


def gpu_run(c, ws=None, **kw):
    """The kernel on a case -> numpy (dets, count, src, members)."""
    from ppyolo_hip import ops
    p = dict(c['kw'])
    p.update(kw)
    dets, count = torch.from_numpy(c['dets']).cuda(), torch.from_numpy(c['count']).cuda()
    tab = ops.fuse_views_table(c['views'])
    w = np.ascontiguousarray(c['weight'], dtype=np.float32)
    n, k = c['n'], p['keep_top_k']
    out = (torch.full((n, k, 6), 7.0, dtype=torch.float32, device='cuda'), torch.full((n,), 7, dtype=torch.int32, device='cuda'),
           torch.full((n, k, 2), 7, dtype=torch.int32, device='cuda'), torch.full((n, k), 7, dtype=torch.int32, device='cuda'))
    ops.fuse_views(dets, count, tab, torch.from_numpy(tab).cuda(), w, torch.from_numpy(w).cuda(), n, p['thresh'], p['score_thresh'],
                   k, *out, ws=ws)
    return tuple(t.cpu().numpy() for t in out)


def same(got, want, what=''):
    for g, w, name in zip(got, want, ('dets', 'count', 'src', 'members')):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g.view(np.int32) != w.view(np.int32))[:4])


def mixed(st):
    """At least one cluster of several rows and one singleton."""
    return st['max_members'] >= 2 and st['singletons'] >= 1


@pytest.mark.parametrize('name', sorted(R.hand_cases()))
def test_hand_cases(name):
    c = R.hand_cases()[name]
    same(gpu_run(c), R.run(c), name)


@pytest.mark.parametrize('V', R.SPREAD_V)
def test_clustered_recipe_dealt_to_views_with_mirrors(V):
    c = R.spread_case(V % 4, V)
    st = []
    want = R.run(c, stats=st)
    assert mixed(st[0]) and (c['views'][:, 3] > 0).sum() == V // 2
    same(gpu_run(c), want, V)
    same(gpu_run(c, thresh=0.3, keep_top_k=40), R.run(c, thresh=0.3, keep_top_k=40), V)


@pytest.fixture(scope='module')
def full_case():
    c = R.uniform_case(*R.BOUNDARIES[-1])
    st = []
    return c, R.run(c, stats=st), st[0]


@pytest.mark.parametrize('rows,V,K', R.BOUNDARIES[:-1])
def test_rows_at_the_stage_boundaries(rows, V, K):
    """A wave's 64-row chunk +-1 and the counting sort's size +-1 (beyond it the bitonic network orders)."""
    assert rows in (63, 64, 65, R.RANK_MAX - 1, R.RANK_MAX, R.RANK_MAX + 1)
    c = R.uniform_case(rows, V, K)
    st = []
    want = R.run(c, stats=st)
    assert st[0]['admitted'] == rows and mixed(st[0])
    same(gpu_run(c), want, rows)


def test_the_most_rows_an_image_may_have_and_the_cut(full_case):
    c, want, st = full_case
    assert st['admitted'] == R.MAX_ROWS and st['clusters'] > 1024 and mixed(st) and want[1][0] == 1024
    same(gpu_run(c), want)
    same(gpu_run(c, keep_top_k=1), tuple(w[:, :1] if w.ndim > 1 else np.minimum(w, 1) for w in want))


def test_one_row_more_is_refused():
    from ppyolo_hip._lib import PPYoloHipError
    rows, V, K = R.T.TOO_MANY
    c = dict(dets=np.zeros((V, K, 6), np.float32), count=np.zeros((V,), np.int32), views=np.zeros((V, 4), np.int32),
             weight=np.ones((V,), np.float32), n=1, kw=dict(thresh=0.5, score_thresh=0.0, keep_top_k=10))
    with pytest.raises(PPYoloHipError, match='3 views x 2731 rows = 8193 rows, at most 8192'):
        gpu_run(c)


@pytest.mark.parametrize('V,K', R.MANY_VIEWS)
def test_many_views_with_padding_views_between(V, K):
    c = R.many_views_case(V, K)
    st = []
    want = R.run(c, stats=st)
    assert mixed(st[0]) and (c['views'][:, 0] == -1).sum() == V // 4
    same(gpu_run(c), want, V)


def test_all_rows_in_one_class():
    c = R.one_class_case()
    st = []
    want = R.run(c, stats=st)
    assert st[0]['admitted'] == 2048 and st[0]['classes'] == 1 and mixed(st[0])
    same(gpu_run(c), want)


def test_rows_spread_over_80_classes():
    c = R.many_classes_case()
    st = []
    want = R.run(c, stats=st)
    assert st[0]['classes'] == 80 and mixed(st[0])
    same(gpu_run(c), want)
    same(gpu_run(c, keep_top_k=1), R.run(c, keep_top_k=1))


def test_second_call_on_a_reused_dirtied_workspace(full_case):
    from ppyolo_hip import ops
    big, want_big, _ = full_case
    ws = ops.fuse_views_workspace(1, 64, 128, 'cuda')
    assert ws.numel() == 64 * 8192
    same(gpu_run(big, ws=ws), want_big)
    for name in ('fused_not_members', 'padding_view', 'left_out'):
        c = R.hand_cases()[name]
        ws[1::3] = 0xff
        same(gpu_run(c, ws=ws), R.run(c), name)
    small = R.spread_case(2, 6, 7)
    ws.fill_(0x7f)
    same(gpu_run(small, ws=ws), R.run(small))
    same(gpu_run(big, ws=ws), want_big)


def test_nan_poisoned_view_beside_a_clean_image():
    c = R.poisoned_case()
    st = []
    want = R.run(c, stats=st)
    assert mixed(st[0]) and mixed(st[1])
    got = gpu_run(c)
    same(got, want)
    assert np.isfinite(got[0]).all()
    alone = R.run(R.spread_case(1, 2, 100))
    assert got[0][1].tobytes() == alone[0][0].tobytes()          # image 1 is what it is alone


def test_two_runs_give_the_same_bytes(full_case):
    for c in (full_case[0], R.spread_case(3, 41)):
        same(gpu_run(c), gpu_run(c))


def test_no_host_synchronisation_and_graph_capture():
    """One launch, capturable: the replayed graph writes what the eager call wrote."""
    from ppyolo_hip import ops
    c = R.spread_case(0, 41)
    p = c['kw']
    dets, count = torch.from_numpy(c['dets']).cuda(), torch.from_numpy(c['count']).cuda()
    tab = ops.fuse_views_table(c['views'])
    d_tab, d_w = torch.from_numpy(tab).cuda(), torch.from_numpy(c['weight']).cuda()
    ws = ops.fuse_views_workspace(1, 41, 100, 'cuda')
    out = (torch.empty((1, 40, 6), dtype=torch.float32, device='cuda'), torch.empty((1,), dtype=torch.int32, device='cuda'),
           torch.empty((1, 40, 2), dtype=torch.int32, device='cuda'), torch.empty((1, 40), dtype=torch.int32, device='cuda'))

    def call():
        ops.fuse_views(dets, count, tab, d_tab, c['weight'], d_w, 1, p['thresh'], p['score_thresh'], 40, *out, ws=ws)
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
                                     (dict(weight=float('nan')), 'view 1: weight nan'), (dict(weight=0.0), 'view 1: weight 0'),
                                     (dict(weight=float('inf')), 'view 1: weight inf'), (dict(weight=-1.0), 'view 1: weight -1'),
                                     (dict(mirror=-1), 'view 1: mirror_w = -1')])
def test_refusals_by_name(kw, word):
    from ppyolo_hip._lib import PPYoloHipError
    c = R.hand_cases()['equal_boxes']
    c = dict(c, views=c['views'].copy(), weight=c['weight'].copy())
    kw = dict(kw)
    if 'weight' in kw:
        c['weight'][1] = kw.pop('weight')
    if 'mirror' in kw:
        c['views'][1, 3] = kw.pop('mirror')
    if 'keep_top_k' in kw:          # (the outputs cannot have the refused shape: any will do, the call ends before it reads them)
        from ppyolo_hip import ops
        dets, count = torch.from_numpy(c['dets']).cuda(), torch.from_numpy(c['count']).cuda()
        tab = ops.fuse_views_table(c['views'])
        out = (torch.empty((1, 1, 6), device='cuda'), torch.empty((1,), dtype=torch.int32, device='cuda'),
               torch.empty((1, 1, 2), dtype=torch.int32, device='cuda'), torch.empty((1, 1), dtype=torch.int32, device='cuda'))
        with pytest.raises(PPYoloHipError, match=word):
            ops.fuse_views(dets, count, tab, torch.from_numpy(tab).cuda(), c['weight'], torch.from_numpy(c['weight']).cuda(), 1, 0.5, 0.0,
                           kw['keep_top_k'], *out)
        return
    with pytest.raises(PPYoloHipError, match=word):
        gpu_run(c, **kw)


def test_refusals_of_the_table_and_the_workspace():
    from ppyolo_hip._lib import PPYoloHipError
    c = R.hand_cases()['equal_boxes']
    bad = dict(c, views=c['views'].copy())
    bad['views'][1, 0] = 1                                   # image 1 of n = 1
    with pytest.raises(PPYoloHipError, match='code -1'):
        gpu_run(bad)
    with pytest.raises(PPYoloHipError, match='workspace'):
        gpu_run(c, ws=torch.empty(16, dtype=torch.uint8, device='cuda'))
    with pytest.raises(PPYoloHipError, match='workspace'):
        gpu_run(c, ws=torch.empty(256 + 8, dtype=torch.uint8, device='cuda')[8:])      # large enough, not 16-byte aligned
    zero_k = dict(c, dets=np.zeros((2, 0, 6), np.float32))
    with pytest.raises(PPYoloHipError, match='K = 0 rows per view'):
        gpu_run(zero_k, ws=torch.empty(64, dtype=torch.uint8, device='cuda'))
    assert gpu_run(c)[1].tolist() == [1]                     # and it still works
