"""multiclass_nms on the GPU (csrc/multiclass_nms.hip) against the float32 numpy restatement (tests/multiclass_nms_ref.py):
dets, count and keep_idx are compared for EQUALITY, bit for bit -- nothing in this operator is transcendental, so there is
no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import multiclass_nms_ref as R
from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config, multiclass_nms_defaults
from ppyolo_hip import synth

pytestmark = pytest.mark.gpu
F = np.float32


def candidates(scores, score_threshold):
    """scores [N, M, C] numpy -> device candidate buffers (key, idx, count), capacity M * C."""
    from ppyolo_hip import ops
    s = torch.from_numpy(np.array(scores, dtype=F)).cuda()
    N, M, C = s.shape
    ck = torch.zeros((N, M * C), dtype=torch.int32, device='cuda')
    ci = torch.zeros((N, M * C), dtype=torch.int32, device='cuda')
    cc = torch.zeros((N,), dtype=torch.int32, device='cuda')
    ops.nms_candidates(s, score_threshold, ck, ci, cc)
    return ck, ci, cc


def nms(boxes, C, cand, nms_top_k, keep_top_k, nms_threshold=0.3, normalized=True, nms_eta=1.0, background_label=-1, ws=None):
    """boxes [N, M, 4] numpy + candidate buffers -> (dets, count, keep_idx) as numpy, as the kernels wrote them."""
    from ppyolo_hip import ops
    b = torch.from_numpy(np.array(boxes, dtype=F)).cuda()
    N = b.shape[0]
    kk = max(int(keep_top_k), 1)
    # poisoned outputs: every row, padding included, must be written by the call
    dets = torch.full((N, kk, 6), 7.0, dtype=torch.float32, device='cuda')
    cnt = torch.full((N,), 77, dtype=torch.int32, device='cuda')
    keep = torch.full((N, kk), 777, dtype=torch.int32, device='cuda')
    ops.multiclass_nms(b, C, cand[0], cand[1], cand[2], nms_top_k, keep_top_k, nms_threshold, normalized, nms_eta,
                       background_label, dets, cnt, keep, ws)
    torch.cuda.synchronize()
    return dets.cpu().numpy(), cnt.cpu().numpy(), keep.cpu().numpy()


def reference(boxes, scores, cfg):
    res = [R.multiclass_nms(boxes[n], scores[n], **cfg) for n in range(boxes.shape[0])]
    return R.padded(res, cfg['keep_top_k'])


def same_bits(got, want, what=''):
    d, c, k = got
    rd, rc, rk = want
    assert np.array_equal(c, rc), '%s: counts %s, expected %s' % (what, c, rc)
    assert np.array_equal(k, rk), '%s: keep_idx differs' % what
    assert d.dtype == np.float32 and rd.dtype == np.float32
    assert np.array_equal(d.view(np.uint32), rd.view(np.uint32)), '%s: dets differ in bits' % what


def run_case(boxes, scores, what='', **cfg):
    """One batch (boxes [N, M, 4], scores [N, M, C]) through nms_candidates + multiclass_nms, compared with the restatement."""
    boxes = np.asarray(boxes, dtype=F)
    scores = np.asarray(scores, dtype=F)
    if boxes.ndim == 2:
        boxes, scores = boxes[None], scores[None]
    full = dict(score_threshold=0.0, nms_top_k=1024, keep_top_k=1024, nms_threshold=0.5, normalized=True)
    full.update(cfg)
    want = reference(boxes, scores, full)
    kernel_cfg = {k: v for k, v in full.items() if k != 'score_threshold'}
    got = nms(boxes, scores.shape[2], candidates(scores, full['score_threshold']), **kernel_cfg)
    same_bits(got, want, what)
    return got


# ---- 3. the hand-derived cases of tests/test_multiclass_nms_ref.py ----

def test_hand_cases():
    two = [[0, 0, 2, 2], [0, 0, 2, 1]]
    sc2 = [[0.9], [0.8]]
    assert run_case(two, sc2, 'exact 0.5', nms_threshold=0.5)[1][0] == 2
    assert run_case(two, sc2, 'below 0.5', nms_threshold=0.49)[1][0] == 1
    assert run_case(two, sc2, '6/9', nms_threshold=0.5, normalized=False)[1][0] == 1
    assert run_case(two, sc2, 'threshold rounded to float32', nms_threshold=2.0 / 3.0, normalized=False)[1][0] == 2
    for normalized in (True, False):
        boxes, scores = R.chain(200)
        d, c, k = run_case(boxes, scores, 'chain', nms_threshold=0.45, normalized=normalized)
        assert c[0] == 100 and list(k[0, :100]) == list(range(0, 200, 2))
        zero = [[1, 1, 1, 1], [1, 1, 1, 1]]
        assert run_case(zero, sc2, 'NaN IoU', normalized=normalized)[1][0] == 1
        inv = [[5, 5, 3, 3], [5, 5, 3, 3]]
        assert run_case(inv, sc2, 'inverted', normalized=normalized)[1][0] == 2
    tie = [[0, 0, 10, 10], [0, 0, 10, 9], [50, 50, 60, 60]]
    assert list(run_case(tie, [[0.5], [0.5], [0.5]], 'tie in a class')[2][0, :2]) == [0, 2]
    far = [[0, 0, 10, 10], [100, 100, 110, 110]]
    sc = [[0.5, 0.5, 0.5], [0.7, 0.0, 0.5]]
    assert list(run_case(far, sc, 'tie at the cut', keep_top_k=3)[2][0]) == [1 * 3 + 0, 0 * 3 + 0, 0 * 3 + 1]
    assert run_case(far, sc, 'output order', keep_top_k=10)[1][0] == 5
    d, c, k = run_case(far, [[0.9, 0.8], [0.7, 0.25]], 'background', background_label=0)
    assert c[0] == 2 and list(d[0, :2, 0]) == [1.0, 1.0]


# ---- 4. / 6. clustered random boxes ----

@pytest.fixture(scope='module')
def clustered():
    data = [R.clustered(seed) for seed in (0, 1, 2)]
    boxes = np.stack([b for b, s in data])
    scores = np.stack([s for b, s in data])
    stats = []
    res = []
    for n in range(3):
        st = {}
        res.append(R.multiclass_nms(boxes[n], scores[n], stats=st, **R.CLUSTERED_CFG))
        stats.append(st)
    want = R.padded(res, R.CLUSTERED_CFG['keep_top_k'])
    for a in (boxes, scores) + want:
        a.setflags(write=False)
    return boxes, scores, stats, want


def _clustered_kernel_cfg():
    return {k: v for k, v in R.CLUSTERED_CFG.items() if k != 'score_threshold'}


def test_clustered_boxes(clustered):
    boxes, scores, stats, want = clustered
    for st in stats:      # the input still exercises truncation, suppression and the keep_top_k cut
        assert st['truncated'] == 5 and 244 <= st['suppressed'] <= 252 and 68 <= st['selected'] <= 76, st
    got = nms(boxes, 5, candidates(scores, R.CLUSTERED_CFG['score_threshold']), **_clustered_kernel_cfg())
    same_bits(got, want, 'clustered')
    assert list(got[1]) == [40, 40, 40]


def test_candidate_order_independence(clustered):
    boxes, scores, stats, want = clustered
    ck, ci, cc = candidates(scores, R.CLUSTERED_CFG['score_threshold'])
    first = nms(boxes, 5, (ck, ci, cc), **_clustered_kernel_cfg())
    again = nms(boxes, 5, (ck, ci, cc), **_clustered_kernel_cfg())
    same_bits(again, first, 'second run on the same buffers')
    rng = np.random.RandomState(7)
    pk, pi = ck.cpu().numpy().copy(), ci.cpu().numpy().copy()
    for n, c in enumerate(cc.cpu().numpy()):
        assert c > 300
        perm = rng.permutation(int(c))
        assert not np.array_equal(perm, np.arange(int(c)))
        pk[n, :c], pi[n, :c] = pk[n, perm], pi[n, perm]
    shuffled = nms(boxes, 5, (torch.from_numpy(pk).cuda(), torch.from_numpy(pi).cuda(), cc), **_clustered_kernel_cfg())
    same_bits(shuffled, first, 'shuffled candidate list')
    same_bits(shuffled, want, 'shuffled candidate list against the restatement')


# ---- 5. boundaries ----

def test_chain_across_ballot_words():
    boxes, scores = R.chain(1500)
    d, c, k = run_case(boxes, scores, 'chain 1500', nms_threshold=0.45, nms_top_k=1024)
    assert c[0] == 512 and list(k[0, :512]) == list(range(0, 1024, 2))


def test_keep_top_k_one(clustered):
    boxes, scores, _, _ = clustered
    d, c, k = run_case(boxes, scores, 'keep_top_k = 1', **dict(R.CLUSTERED_CFG, keep_top_k=1))
    assert list(c) == [1, 1, 1] and d.shape == (3, 1, 6)


def test_empty_image_between_two_and_single_candidate_class(clustered):
    boxes, scores, _, _ = clustered
    scores = scores.copy()
    scores[1] = 0.0                                   # image 1: no candidate at all
    scores[2, :, 3] = 0.0                             # image 2, class 3: exactly one candidate
    scores[2, 17, 3] = 0.6
    d, c, k = run_case(boxes, scores, 'empty image', **dict(R.CLUSTERED_CFG, keep_top_k=200))
    assert c[0] > 40 and c[1] == 0 and c[2] > 40
    assert (d[1] == -1).all() and (k[1] == -1).all()
    assert list(k[2]).count(17 * 5 + 3) == 1 and (d[2, :c[2], 0] == 3).sum() == 1


def _spread(seed, M, C, extent):
    """M boxes of 20..80 px spread over [0, extent]^2: suppression is the exception, the selected lists get long."""
    r = np.random.RandomState(seed)
    ctr = r.uniform(0, extent, size=(M, 2))
    size = r.uniform(20, 80, size=(M, 2))
    boxes = np.concatenate([ctr - size / 2, ctr + size / 2], axis=1).astype(F)
    scores = r.uniform(-0.5, 1, size=(M, C)).astype(F)
    return boxes, scores


def test_all_pass_list_larger_than_lds_stage():
    """score_threshold = -1: every (box, class) pair is a candidate, 12 000 per image -- more than the 8192 entries the
    select kernels stage in LDS."""
    data = [R.clustered(10 + n, M=3000, C=4) for n in range(2)]
    boxes, scores = np.stack([b for b, s in data]), np.stack([s for b, s in data])
    d, c, k = run_case(boxes, scores, 'all-pass', score_threshold=-1.0, nms_top_k=100, keep_top_k=100, nms_threshold=0.45,
                       normalized=False)
    assert (c > 10).all()


def test_class_larger_than_its_lds_stage():
    """One class with more candidates (5000, negative scores included) than the 4096 keys a class stages in LDS: the select
    walks the global list; the selected list grows past one stride of the 16 waves."""
    boxes, scores = _spread(3, 5000, 2, 1500.0)
    d, c, k = run_case(boxes, scores, 'large class', score_threshold=-1.0, nms_top_k=1024, keep_top_k=1024,
                       nms_threshold=0.3, normalized=False)
    assert c[0] == 1024 and 100 < (d[0, :, 0] == 0).sum() < 1000


def test_merged_list_larger_than_lds_stage():
    """12 classes x ~900 selections: the keep_top_k cut runs its radix select on more than 8192 merged entries."""
    boxes, scores = _spread(4, 1024, 12, 6000.0)
    st = {}
    R.multiclass_nms(boxes, scores, -1.0, 1024, 1000, 0.3, False, stats=st)
    assert st['selected'] > 8192 and st['suppressed'] > 0, st
    d, c, k = run_case(boxes, scores, 'large merge', score_threshold=-1.0, nms_top_k=1024, keep_top_k=1000,
                       nms_threshold=0.3, normalized=False)
    assert c[0] == 1000


# ---- 7. what is refused ----

def test_unsupported_parameters_and_workspace(clustered):
    from ppyolo_hip import ops
    from ppyolo_hip._lib import PPYoloHipError
    boxes, scores, _, _ = clustered
    cand = candidates(scores, 0.05)
    base = dict(nms_top_k=64, keep_top_k=40, nms_threshold=0.45, normalized=False)
    ws = ops.multiclass_nms_workspace(3, 5, 64, 1000, 'cuda')
    for key, val in (('nms_top_k', 0), ('nms_top_k', 1025), ('keep_top_k', 0), ('nms_eta', 0.9), ('keep_top_k', 1025),
                     ('nms_top_k', -1), ('keep_top_k', -1)):
        with pytest.raises(PPYoloHipError, match=key):
            nms(boxes, 5, cand, ws=ws, **dict(base, **{key: val}))
    assert ws.numel() * 4 == 16 + 3 * 5 * 64 * 8
    with pytest.raises(PPYoloHipError, match='workspace'):
        nms(boxes, 5, cand, ws=ws[:ws.numel() - 4], **base)
    same_bits(nms(boxes, 5, cand, ws=ws, **base), nms(boxes, 5, cand, **base), 'caller-owned workspace')


# ---- 8. end to end ----

def _key_to_score(key):
    k = key.astype(np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k)
    return bits.astype(np.uint32).view(np.float32)


def _restatement_on_executor_buffers(ex, nms_cfg, C):
    """The restatement applied to the executor's OWN decoded boxes and candidate scores (read back after a forward): isolates
    the NMS from decode rounding."""
    boxes = ex.boxes.cpu().numpy()
    N, M = boxes.shape[:2]
    cnt = ex.cand_count.cpu().numpy()
    key, idx = ex.cand_key.cpu().numpy(), ex.cand_idx.cpu().numpy()
    cfg = {k: v for k, v in nms_cfg.items() if k != 'nms_type'}
    res = []
    for n in range(N):
        scores = np.full((M * C,), -np.inf, dtype=F)          # not a candidate: never above the threshold
        scores[idx[n, :cnt[n]]] = _key_to_score(key[n, :cnt[n]])
        assert (scores[idx[n, :cnt[n]]] > F(cfg['score_threshold'])).all()
        res.append(R.multiclass_nms(boxes[n], scores.reshape(M, C), **cfg))
    return R.padded(res, cfg['keep_top_k']), cnt


@pytest.mark.parametrize('cfgc,S', [(PPYOLO_r18vd_Config, 64), (PPYOLO_2x_Config, 96)])
def test_end_to_end(cfgc, S, golden, monkeypatch):
    cfg = cfgc()
    cfg.nms_cfg = multiclass_nms_defaults()
    x = synth.synth_images(2, S, seed=1234).cuda()
    ims = torch.tensor([[480., 640.], [375., 500.]]).cuda()
    runs = {}
    for graph in ('1', '0'):
        monkeypatch.setenv('PPYOLO_HIP_GRAPH', graph)
        model, sd = build_model(cfg, 0, 'cuda')
        preds = [p.clone() for p in model(x, ims)]
        dets, cnt, keep = [t.clone() for t in model.forward_padded(x, ims)]      # (graph = 1: a replay)
        runs[graph] = (dets.cpu().numpy(), cnt.cpu().numpy(), keep.cpu().numpy())
        if graph == '1':
            ex = model._plans.executor(x)
            assert ex.graph is not None, 'the forward with multiclass_nms was captured into a graph'
            want, ncand = _restatement_on_executor_buffers(ex, cfg.nms_cfg, cfg.num_classes)
            assert ncand.min() > 0, 'the synthetic model produced no candidates: the comparison would be empty'
            same_bits(runs[graph], want, 'forward against the restatement on the executor\'s buffers')
            # forward() and forward_padded() conventions: [K, 6] per image or the [[-1] * 6] row; -1 padding behind count
            for i, p in enumerate(preds):
                k = int(cnt[i])
                assert tuple(p.shape) == (max(k, 1), 6)
                assert torch.equal(p, dets[i, :max(k, 1)])
                assert bool((dets[i, k:] == -1).all()) and bool((keep[i, k:] == -1).all()) and bool((keep[i, :k] >= 0).all())
            assert dets.shape == (2, 100, 6) and int(cnt.max()) > 0
            # in_flight(2): two lanes, each its own executor, workspace and graph
            pipe = model.in_flight(2)
            x2 = synth.synth_images(2, S, seed=77).cuda()
            want2 = [p.clone() for p in model(x2, ims)]
            t1, t2 = pipe.submit(x, ims), pipe.submit(x2, ims)
            for a, b in zip(t2.result() + t1.result(), want2 + preds):
                assert torch.equal(a, b), 'in_flight(2) differs from model()'
    same_bits(runs['0'], runs['1'], 'eager against graph')
    # the default configuration is untouched by all this: Matrix-NMS, head outputs as the golden of this size has them,
    # detections as the CPU oracle computes them
    from oracle import ppyolo_oracle as orc
    from ppyolo_hip.runtime import build_plan
    from ppyolo_hip.engine import HipExecutor
    g = golden('g6_r18vd_64' if S == 64 else 'g6_r50vd_96')
    assert [int(v) for v in g['meta']] == [S, 2, 0, 1234]
    dcfg = cfgc()
    assert dcfg.nms_cfg['nms_type'] == 'matrix_nms'
    dmodel, dsd = build_model(dcfg, 0, 'cuda')
    plan = build_plan(dmodel, 2, S, S, torch.device('cuda'))
    assert plan.decode['nms_type'] == 'matrix_nms'
    dex = HipExecutor(plan, 'cuda', use_graph=False)
    dex.set_inputs(x, synth.synth_im_size(2).cuda())
    dex.run()
    torch.cuda.synchronize()
    for i, a in enumerate(plan.head_outs):
        got, ref = dex.view(a).dense().permute(0, 3, 1, 2).cpu(), torch.from_numpy(g['out%d' % i])
        assert (got - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
    from test_gpu_model import _check_preds
    mine = dmodel(x, ims)
    keep = dmodel.forward_padded(x, ims)[2]
    oracle = orc.ppyolo_forward(dsd, dcfg, x.cpu(), ims.cpu(), return_index=True)
    _check_preds(mine, [o[0] for o in oracle], keep, [o[1] for o in oracle])
