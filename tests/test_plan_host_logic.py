"""Host-side logic of the product, checked on CPU: the plan the HIP executor replays
(BN fold, KRSC weights, concat slices, CoordConv bias maps, fused residual / upsample, DCN
column order, decode parameters) is interpreted with reference ops (tests/plan_interp.py) and
must reproduce the oracle and the reference-generated goldens."""
import numpy as np
import pytest
import torch

from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from oracle import ppyolo_oracle as orc
from plan_interp import CpuPlanRunner
from ppyolo_hip import synth
from ppyolo_hip.engine import A
from ppyolo_hip.runtime import build_plan

TOL = 2e-4   # BN folded into scale/shift + coord terms summed separately -> fp32 roundoff only


@pytest.mark.parametrize('tag,cfgc', [('r18vd_64', PPYOLO_r18vd_Config), ('r50vd_96', PPYOLO_2x_Config)])
def test_plan_matches_golden_features(golden, tag, cfgc):
    g = golden('g6_' + tag)
    S, N, seed, iseed = [int(v) for v in g['meta']]
    cfg = cfgc()
    model, sd = build_model(cfg, seed)
    plan = build_plan(model, N, S, S, 'cpu')
    feats, outs, _ = CpuPlanRunner(plan).run(synth.synth_images(N, S, seed=iseed))
    for i, f in enumerate(feats):
        ref = torch.from_numpy(g['feat%d' % i])
        assert f.shape == ref.shape
        assert (f - ref).abs().max() <= TOL * max(1.0, ref.abs().max().item()), (tag, 'feat', i)
    for i, o in enumerate(outs):
        ref = torch.from_numpy(g['out%d' % i])
        assert (o - ref).abs().max() <= TOL * max(1.0, ref.abs().max().item()), (tag, 'out', i)


@pytest.mark.parametrize('tag,cfgc', [('r18vd_320', PPYOLO_r18vd_Config), ('r50vd_160', PPYOLO_2x_Config)])
def test_plan_end_to_end_matches_golden(golden, tag, cfgc):
    g = golden('g7_' + tag)
    S, N, seed, iseed = [int(v) for v in g['meta']]
    cfg = cfgc()
    model, sd = build_model(cfg, seed)
    plan = build_plan(model, N, S, S, 'cpu')
    im_size = torch.from_numpy(g['im_size'])
    _, outs, preds = CpuPlanRunner(plan).run(synth.synth_images(N, S, seed=iseed), im_size)
    for i, p in enumerate(preds):
        ref = torch.from_numpy(g['pred%d' % i])
        assert p.shape == ref.shape
        assert torch.equal(p[:, 0], ref[:, 0])                         # labels, in order
        assert (p[:, 1] - ref[:, 1]).abs().max() <= 1e-4               # scores
        # boxes: 1e-3 px, or 2e-5 of the box side for large boxes -- the plan folds BatchNorm scales into the weights of the four
        # projection-shortcut layers (model/resnet_vd.py), i.e. it rounds in another order than the reference's eager ops, and a
        # box edge moves by (logit noise) x (box side) / 2: what the reference does against itself (tests/golden/g18_*: 1e-5)
        side = torch.maximum(ref[:, 4] - ref[:, 2], ref[:, 5] - ref[:, 3]).clamp_min(1.0)
        assert bool(((p[:, 2:] - ref[:, 2:]).abs().max(dim=1).values <= torch.clamp(2e-5 * side, min=1e-3)).all())


def test_plan_structure_r50():
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg)
    plan = build_plan(model, 2, 160, 160, 'cpu')
    kinds = [o['op'] for o in plan.ops]
    # (74 = 78 - the four projection-shortcut launches, folded into their block's conv3: ConvBlock._emit_folded)
    assert kinds.count('conv') == 74 and kinds.count('dcn') == 3 and kinds.count('spp') == 1
    assert kinds.count('stem') == 1 and kinds.count('maxpool') == 1 and kinds.count('avgpool') == 3
    assert len(plan.setup_ops) == 12                # one CoordConv bias map per coord conv
    # every conv reads a 32-channel-aligned, 16-byte aligned slice
    for o in plan.ops:
        if o['op'] == 'conv':
            assert o['x'].C % 32 == 0 and o['x'].coff % 4 == 0
    d = plan.decode
    assert d['M_total'] == 3 * (5 * 5 + 10 * 10 + 20 * 20)
    assert [len(l['anchors']) for l in d['levels']] == [3, 3, 3]
    assert d['levels'][0]['anchors'][0] == [116.0, 90.0] and d['levels'][2]['downsample'] == 8


def test_cpu_input_raises():
    from ppyolo_hip._lib import PPYoloHipError
    model, _ = build_model(PPYOLO_r18vd_Config())
    with pytest.raises(PPYoloHipError):
        model(torch.zeros(1, 3, 64, 64), torch.tensor([[64., 64.]]))


def test_pool_links_of_the_r50_plan():
    """plan_links.link_pools: the average pools in front of the stage-3 and stage-4
    projection shortcuts go to the 1x1 convolutions that produce their inputs (C64 -> K256 and C128 -> K512, the latter into a
    slice of the stage-3 / route buffer that has a second writer), the one in front of stage 5 (input from a C = 256 layer) stays
    a launch of its own; nothing is linked without f16x2 operands; the linked plan still interprets to the same features."""
    from ppyolo_hip.plan_links import BufferIndex, link_pools, op_io
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg)
    plan = build_plan(model, 2, 160, 160, 'cpu')
    x = synth.synth_images(2, 160, seed=3)
    base_feats, base_outs, _ = CpuPlanRunner(plan).run(x)
    assert link_pools(BufferIndex(plan.ops), lambda c: False) == 0
    assert link_pools(BufferIndex(plan.ops), lambda c: True) == 2
    pools = [o for o in plan.ops if o['op'] == 'avgpool']
    assert [o.get('owner') is not None for o in pools] == [True, True, False]
    for o, (C, Kout) in zip(pools[:2], ((64, 256), (128, 512))):
        c = o['owner']
        assert tuple(c['w'].shape) == (Kout, 1, 1, C) and c['pool'] is o['y']
        assert (c['y'].buf, c['y'].coff, c['y'].C) == (o['x'].buf, o['x'].coff, o['x'].C) and c['res'] is not None
    assert op_io(pools[0]) == ([], []) and pools[0]['y'].buf in op_io(pools[0]['owner'])[1]
    feats, outs, _ = CpuPlanRunner(plan).run(x)             # (the interpreter pools where the plan says; same tensors)
    for a, b in zip(feats + outs, base_feats + base_outs):
        assert torch.equal(a, b)


def test_maxpool_link_of_the_stem():
    """plan_links.link_maxpools: the stem's MaxPool2d(3, 2, 1) goes to the convolution in
    front of it (conv1_3: 3x3, C32 -> K64), whose launch then writes only the pooled tensor -- in the R50vd plan into the channel slice
    of the first block's wide buffer; nothing is linked without f16x2 operands, and nothing when somebody else reads the tensor."""
    from ppyolo_hip.plan_links import BufferIndex, link_maxpools, op_io
    for cfgc in (PPYOLO_2x_Config, PPYOLO_r18vd_Config):
        model, _ = build_model(cfgc())
        plan = build_plan(model, 2, 160, 160, 'cpu')
        assert link_maxpools(BufferIndex(plan.ops), set(), lambda c: False) == 0
        mp = [o for o in plan.ops if o['op'] == 'maxpool']
        assert len(mp) == 1
        assert link_maxpools(BufferIndex(plan.ops), {mp[0]['x'].buf}, lambda c: True) == 0          # (a pinned tensor must exist)
        assert link_maxpools(BufferIndex(plan.ops), set(), lambda c: True) == 1
        c = mp[0]['owner']
        assert tuple(c['w'].shape) == (64, 3, 3, 32) and c['mpool'] is mp[0]['y'] and c['act'] == 'relu'
        assert op_io(mp[0]) == ([], [])
        assert op_io(c) == ([c['x'].buf], [mp[0]['y'].buf])          # the full-resolution buffer is not written any more
        del c['mpool'], mp[0]['owner']


def test_split_pairs_of_the_r50_plan():
    """plan_links.split_pairs (the structural part of HipExecutor._link_splits): which tensors of the R50vd plan may travel pre-split.
    Every bottleneck's conv1 -> conv2 except where the DCNv2 reads conv1's output too (stage 5) -- 13 pairs; conv2 -> conv3
    (the 3x3's output has one reader) -- 13 more; the stem's conv2 -> conv3; the head's chains, incl. the two routes with two
    readers and the tips feeding the output convolutions.  Never a feature map, a head output, a shortcut operand, a pooled or
    upsampled tensor; nothing without f16x2 operands."""
    from ppyolo_hip.plan_links import BufferIndex, op_io, split_pairs
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg)
    plan = build_plan(model, 2, 160, 160, 'cpu')
    pinned = {a.buf for a in list(plan.head_outs) + list(plan.feats)}
    index = BufferIndex(plan.ops)
    assert split_pairs(index, plan.buffers, pinned, lambda c: False) == []
    pairs = split_pairs(index, plan.buffers, pinned, lambda c: True)
    only3 = split_pairs(index, plan.buffers, pinned, lambda c: True, True)
    shape = lambda o: tuple(o['w'].shape)
    for pr, cons in pairs:
        b = pr['y'].buf
        assert pr['op'] == 'conv' and pr['res'] is None and not pr['ups'] and b not in pinned and plan.buffers[b][3] % 32 == 0
        for c in cons:
            assert c['op'] == 'conv' and c['x'].buf == b and c['x'].C == plan.buffers[b][3] and (c['res'] is None or c['res'].buf != b)
        # nobody else touches the buffer
        for o in plan.ops:
            ins, outs = op_io(o)
            assert (b not in ins or any(o is c for c in cons)) and (b not in outs or o is pr)
    cons3 = [c for _, cs in pairs for c in cs if shape(c)[1] == 3]
    n3 = sum(1 for o in plan.ops if o['op'] == 'conv' and shape(o)[1] == 3)
    # all 3x3 launches but the three conv_offset (their input is shared with the DCNv2 launch) and the stem's second layer (its
    # input comes from the stem kernel, which is no 'conv' op)
    # (42 = 45 - the conv2 -> conv3 links of the first blocks of stages 2-4: their buffer now has a second writer, the shortcut operand)
    assert n3 == 27 and len(cons3) == 23 and len(pairs) == 42
    assert all(shape(c)[1] == 3 for _, cs in only3 for c in cs) and sum(len(cs) for _, cs in only3) <= len(cons3)
    two = [(pr, cs) for pr, cs in pairs if len(cs) == 2]
    assert len(two) == 2 and all(sorted(shape(c)[1] for c in cs) == [1, 3] for _, cs in two)      # the routes of levels 0 and 1
    # chains: an op can be consumer and producer
    prods = {id(pr) for pr, _ in pairs}
    assert any(id(c) in prods for _, cs in pairs for c in cs)


def test_b2b_pairs_of_the_r50_plan():
    """plan_links.b2b_pairs (round 5): conv2 -> conv3 of the two IDENTITY bottlenecks of stage 2
    (64 -> 64 3x3, 64 -> 256 1x1 with the shortcut) run as one launch; not the stage's first block (its conv3 is the folded
    128-channel one), not the deeper stages, nothing in r18vd.  With a pair marked, its first launch reads the shortcut and writes
    the block's output (and the pooled twin), the second does nothing, and conv1 -> conv2 stays a pre-split pair."""
    from ppyolo_hip.plan_links import BufferIndex, b2b_pairs, op_io, split_pairs
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg)
    plan = build_plan(model, 2, 160, 160, 'cpu')
    pinned = {a.buf for a in list(plan.head_outs) + list(plan.feats)}
    index = BufferIndex(plan.ops)
    assert b2b_pairs(index, plan.buffers, pinned, lambda c: False) == []
    pairs = b2b_pairs(index, plan.buffers, pinned, lambda c: True)
    assert len(pairs) == 2
    for a, b in pairs:
        assert tuple(a['w'].shape) == (64, 3, 3, 64) and tuple(b['w'].shape) == (256, 1, 1, 64) and b['res'] is not None
        assert b['x'].buf == a['y'].buf and a['y'].buf not in pinned
    n_before = len(split_pairs(index, plan.buffers, pinned, lambda c: True))
    for a, b in pairs:
        a['b2b'], b['b2b_of'] = b, a
        assert op_io(b) == ([], [])
        ins, outs = op_io(a)
        assert ins == [a['x'].buf, b['res'].buf] and outs[0] == b['y'].buf
    after = split_pairs(BufferIndex(plan.ops), plan.buffers, pinned, lambda c: True)          # (an index of the plan as it is now linked)
    # the two conv2 -> conv3 tensors are gone as links (never written), the conv1 -> conv2 links of those blocks stay
    assert len(after) == n_before - 2
    assert all(any(any(c is a for c in cs) for _, cs in after) for a, _ in pairs)
    for a, b in pairs:
        del a['b2b'], b['b2b_of']
    cfg18 = PPYOLO_r18vd_Config()
    m18, _ = build_model(cfg18)
    p18 = build_plan(m18, 2, 160, 160, 'cpu')
    assert b2b_pairs(BufferIndex(p18.ops), p18.buffers, set(), lambda c: True) == []


def test_tracked_maximum_blocks_of_the_r50_plan():
    """plan_links.assign_amax (round 6, the round-5 advisor's aliasing): the wide buffer
    [conv2 output | pooled block input] of a stage's first block (the folded projection shortcut, model/resnet_vd.py:27-33) has a
    block of its OWN for what conv2 / the DCNv2 launch writes and keeps the block of the tensor it was pooled from as a second,
    read-only one: the fused 1x1 reads both, and NO other reader of the block input -- the head's C3 / C4 convolutions, conv1 of
    the block itself -- sees a block that conv2 writes into."""
    from ppyolo_hip.plan_links import assign_amax
    cfg = PPYOLO_2x_Config()
    model, _ = build_model(cfg)
    plan = build_plan(model, 2, 160, 160, 'cpu')
    n = assign_amax(plan.ops)
    convs = [o for o in plan.ops if o['op'] in ('conv', 'dcn')]
    assert n > 0 and all(o['amax_out_id'] is not None and 0 <= o['amax_out_id'] < n for o in convs)
    two = [o for o in convs if o.get('amax_in2_id') is not None]
    # the four fused conv3 launches (C = 128, 384, 768, 1536), and stage 2's conv1, which reads the pooled half of the same buffer
    fused = [o for o in two if o['x'].C == plan.buffers[o['x'].buf][3]]
    assert sorted(o['x'].C for o in fused) == [128, 384, 768, 1536] and all(tuple(o['w'].shape)[1:3] == (1, 1) for o in fused)
    writers = {}
    for o in convs:
        writers.setdefault(o['amax_out_id'], []).append(o)
    for o in fused:
        assert o['amax_in_id'] != o['amax_in2_id']
        # the own block is written by conv2 (a 3x3 or the DCNv2 launch) only; the second block by the producers of the block INPUT only
        assert all(w['y'].buf == o['x'].buf for w in writers[o['amax_in_id']])
        assert all(w['y'].buf != o['x'].buf for w in writers.get(o['amax_in2_id'], []))
    # the head's readers of C3 / C4 (feature maps; concat buffers with the upsampled routes) scale by their own producers' maxima
    feat_bufs = {a.buf for a in plan.feats}
    for o in convs:
        if o['x'].buf in feat_bufs and o.get('amax_in2_id') is None:
            assert all(w['y'].buf == o['x'].buf for w in writers[o['amax_in_id']]), 'a foreign writer merges into a feature map\'s block'
    # pooled tensors still inherit: every reader of a buffer that holds ONLY a pooled tensor has its source's block
    for o in plan.ops:
        if o['op'] in ('avgpool', 'maxpool'):
            for c in convs:
                if c['x'].buf == o['y'].buf:
                    assert c['amax_in_id'] is not None


def test_dcn_configuration_ids_and_weight_prep_descriptor_layout():
    """Host-side bookkeeping of round 3 that needs no device: (1) the fused-DCNv2 ids -- [0, 18) = scheme * 6 + four-wave tile, from
    18 the eight-wave f16x2 tiles -- as ops.dcnv2_scheme / dcnv2_configs hand them to the plan and the tuner; every committed
    'dcnf' table entry names an id of its own table's scheme.  (2) ops._WeightPrep mirrors PpyWeightPrep of include/ppyolo_hip.h
    field for field (six pointers, six ints: 72 bytes) -- the table is copied to the device as raw bytes."""
    import ctypes
    import json
    import os
    import re
    from ppyolo_hip import ops
    n = ops.dcnv2_num_configs()
    assert n > 3 * ops.DCN_TILES_4W
    assert [ops.dcnv2_scheme(c) for c in (0, 5, 6, 11, 12, 17, 18, n - 1)] == ['fp32', 'fp32', 'bf16x3', 'bf16x3', 'f16x2', 'f16x2', 'f16x2', 'f16x2']
    assert ops.dcnv2_configs('fp32') == list(range(6)) and ops.dcnv2_configs('bf16x3') == list(range(12))
    assert ops.dcnv2_configs('f16x2') == list(range(18)) + list(range(18, n))
    here = os.path.join(os.path.dirname(ops.__file__))
    for mode, fname in (('fp32', 'tuned_gfx950.json'), ('bf16x3', 'tuned_gfx950_bf16x3.json'), ('f16x2', 'tuned_gfx950_f16x2.json')):
        with open(os.path.join(here, fname)) as fh:
            table = json.load(fh)
        ids = [v[0] for k, v in table.items() if k.startswith('dcnf')]
        assert ids and all(c in ops.dcnv2_configs(mode) for c in ids), (mode, ids)
    # the descriptor: same fields, same order, same size as the C struct
    fields = [f for f, _ in ops._WeightPrep._fields_]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(here)), 'include', 'ppyolo_hip.h')).read()
    body = hdr[hdr.index('typedef struct PpyWeightPrep {'):hdr.index('} PpyWeightPrep;')]
    names = re.findall(r'[\s\*](\w+)(?=[,;])', body.split('{', 1)[1])
    assert names == fields, (names, fields)
    assert ctypes.sizeof(ops._WeightPrep) == 6 * 8 + 6 * 4
    assert ops.PREP_SPLIT == int(re.search(r'#define PPY_PREP_SPLIT (\d+)', hdr).group(1))


# ---- plan_links.decide_links / sync_plan on hand-made plans: a three-entry tile table instead of the library's descriptors ----
_Cfg = __import__('collections').namedtuple('_Cfg', 'reads_presplit writes_presplit splitk_mode')
PLAIN, BOTH, READS = 0, 1, 2          # tile ids of the table: neither form / reads and writes pre-split / reads it only
_cfg_of = [_Cfg(0, 0, 'workspace'), _Cfg(1, 1, 'workspace'), _Cfg(1, 0, 'workspace')].__getitem__


def _w(Kout, C, R):
    return torch.empty((Kout, C, R, R), dtype=torch.float32, device='meta')


def _bottleneck(b, x, cfgs, res=None):
    """conv1 1x1 256 -> 64, conv2 3x3 64 -> 64, conv3 1x1 64 -> 256 + shortcut, ReLU each (an identity bottleneck of stage 2)."""
    t = b.conv(x, _w(64, 256, 1), None, None, act='relu')
    t = b.conv(t, _w(64, 64, 3), None, None, act='relu')
    y = b.conv(t, _w(256, 64, 1), None, None, act='relu', res=x if res is None else res)
    for op, c in zip(b.plan.ops[-3:], cfgs):
        op['cfg'], op['splitk'] = c, 1
    return y


def _decide(plan, **kw):
    from ppyolo_hip.plan_links import BufferIndex, decide_links
    return decide_links(plan.ops, BufferIndex(plan.ops), plan.buffers, set(), lambda c: True, _cfg_of, **kw)


def test_decide_links_unfuses_only_the_pair_without_its_input():
    """A fused conv2 -> conv3 pair needs conv2's input pre-split.  conv1 on a tile that cannot write that form: the pair falls back
    to two launches, the link its stand-alone form allows (conv2 -> conv3) is made, and that takes two derivations.  A second
    pair whose conv1 does write pre-split stays fused through it: only the pair without its input falls back."""
    from ppyolo_hip.engine import Builder
    b = Builder(2, 16, 16, 'cpu', skeleton=True)
    x = b.new_act(2, 16, 16, 256)
    y = _bottleneck(b, x, (READS, BOTH, BOTH))
    assert _decide(b.plan) == ([(1, [2])], [], 2)
    assert _decide(b.plan, b2b=False) == ([(1, [2])], [], 1)
    assert _decide(b.plan, rejected=(1,)) == ([(1, [2])], [], 1)
    _bottleneck(b, y, (BOTH, PLAIN, PLAIN))           # (a fused conv2 reads finished operands whatever its own tile)
    assert _decide(b.plan) == ([(1, [2]), (3, [4])], [(4, 5)], 2)
    assert _decide(b.plan, presplit=False) == ([], [], 2)          # (no links at all: no pair gets its input)
    b.plan.ops[0]['cfg'] = BOTH
    assert _decide(b.plan) == ([(0, [1]), (3, [4])], [(1, 2), (4, 5)], 1)
    b.plan.ops[0]['splitk'] = 2           # (partial sums through memory: that launch writes plain fp32)
    assert _decide(b.plan) == ([(1, [2]), (3, [4])], [(4, 5)], 2)


def test_decide_links_all_readers_or_none():
    """A route with two readers -- the tip 3x3 and the 1x1 in front of the upsampling: one of them on a tile that cannot read
    pre-split tensors and neither is linked; the tensor has one form."""
    from ppyolo_hip.engine import Builder
    b = Builder(2, 16, 16, 'cpu', skeleton=True)
    r = b.conv(b.new_act(2, 16, 16, 128), _w(64, 128, 1), None, None, act='relu')
    b.conv(r, _w(128, 64, 3), None, None, act='relu')
    b.conv(r, _w(32, 64, 1), None, None, act='relu', ups=True)
    for op, c in zip(b.plan.ops, (BOTH, BOTH, PLAIN)):
        op['cfg'], op['splitk'] = c, 1
    assert _decide(b.plan) == ([], [], 1)
    b.plan.ops[2]['cfg'] = READS
    assert _decide(b.plan) == ([(0, [1, 2])], [], 1)
    b.plan.ops[1]['splitk'] = 4
    assert _decide(b.plan) == ([], [], 1)


def test_sync_plan_follows_the_fused_pair():
    """The shortcut operand of conv3 is written on the side stream.  Two launches: conv3 waits for that writer.  conv2 -> conv3
    fused: the pair's launch is conv2's, so conv2 waits for it and the absorbed conv3 for nothing."""
    from ppyolo_hip.engine import Builder
    from ppyolo_hip.plan_links import sync_plan
    b = Builder(2, 16, 16, 'cpu', skeleton=True)
    x = b.new_act(2, 16, 16, 256)
    with b.side():
        sc = b.conv(x, _w(256, 256, 1), None, None)
    _bottleneck(b, x, (BOTH, BOTH, BOTH), res=sc)
    ops = b.plan.ops
    assert [o['stream'] for o in ops] == [1, 0, 0, 0]
    assert sync_plan(ops, True) == ([[], [], [], [0]], {0}, 0)
    assert sync_plan(ops, False) == ([[], [], [], []], set(), None)
    links, fused, _ = _decide(b.plan)
    assert fused == [(2, 3)] and links == [(1, [2])]
    ops[2]['b2b'], ops[3]['b2b_of'] = ops[3], ops[2]
    assert sync_plan(ops, True) == ([[], [], [0], []], {0}, 0)


def test_no_link_on_an_op_with_two_tracked_maximum_blocks():
    """Only the plain convolution entry point takes a second tracked-maximum block: the link rules leave an op that carries
    'amax_in2_id' a launch of its own (HipExecutor._run_op would refuse it at the first launch).  The committed plans have no
    such link to lose -- same counts as above with the blocks assigned; a synthetic plan in which the rule bites."""
    from ppyolo_hip.engine import Builder
    from ppyolo_hip.plan_links import BufferIndex, assign_amax, b2b_pairs, link_maxpools, link_pools
    yes = lambda c: True
    for cfgc, want in ((PPYOLO_2x_Config, (2, 1, 2)), (PPYOLO_r18vd_Config, (0, 1, 0))):
        model, _ = build_model(cfgc())
        plan = build_plan(model, 2, 160, 160, 'cpu')
        pinned = {a.buf for a in list(plan.head_outs) + list(plan.feats)}
        assert assign_amax(plan.ops) > 0
        n_pool = link_pools(BufferIndex(plan.ops), yes)
        n_mpool = link_maxpools(BufferIndex(plan.ops), pinned, yes)
        pairs = b2b_pairs(BufferIndex(plan.ops), plan.buffers, pinned, yes)
        for a, b in pairs:
            a['b2b'], b['b2b_of'] = b, a
        assert (n_pool, n_mpool, len(pairs)) == want
        two = [o for o in plan.ops if o.get('amax_in2_id') is not None]
        assert (len(two) > 0) == (cfgc is PPYOLO_2x_Config)
        assert not any(o.get(k) is not None for o in two for k in ('pool', 'mpool', 'b2b', 'b2b_of'))
    # [c1's output | the 2x2 average of c0's]: P reads both halves (two blocks), and its output is pooled
    b = Builder(2, 16, 16, 'cpu', skeleton=True)
    t0 = b.conv(b.new_act(2, 16, 16, 32), _w(32, 32, 1), None, None)
    wide = A(b.new_buf(2, 8, 8, 64), 0, 64, 2, 8, 8)
    b.avgpool(t0, out=b.slice(wide, 32, 32))
    b.conv(b.new_act(2, 8, 8, 32), _w(32, 32, 1), None, None, out=b.slice(wide, 0, 32))
    b.avgpool(b.conv(wide, _w(256, 64, 1), None, None))
    P, pool = b.plan.ops[-2:]
    assign_amax(b.plan.ops)
    assert P['amax_in2_id'] is not None and P['amax_in_id'] not in (None, P['amax_in2_id'])
    assert link_pools(BufferIndex(b.plan.ops), yes) == 0 and pool.get('owner') is None and P.get('pool') is None
    P['amax_in2_id'] = None          # (the same convolution with one block is linked: the rule is what kept it apart)
    assert link_pools(BufferIndex(b.plan.ops), yes) == 1 and pool['owner'] is P


def test_committed_table_on_the_bench_plan():
    """The whole derivation for the flagship workload (R50vd, 8 x 608 x 608, f16x2) without a device: tracked maxima, the
    structural links, the committed tuned_gfx950_f16x2.json through plan_links.apply_tuned, and decide_links over the library's
    own tile descriptors.  Expected: 39 ops with 'x_split', 2 with 'b2b', each of those two with its 'x_split' -- read at commit
    27ed7c5 (the last one that derived its links inside the executor) from that executor's own methods (_assign_amax, _link_pools,
    _link_maxpools, _mark_split_candidates, its table lookup, _link_splits) run over this plan with the executor object standing
    on the CPU; NOT yet read from an executor on an MI355X, as the issue asks -- to be confirmed there."""
    import json
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import ops as K
    from ppyolo_hip import plan_links as L
    from ppyolo_hip.engine import _TUNED_PATHS
    model, _ = build_model(PPYOLO_2x_Config())
    plan = build_plan(model, 8, 608, 608, 'cpu')
    for op in plan.ops:
        if op['op'] in ('conv', 'dcn'):
            op['wf16'] = True           # (the executor's split fp16 weights: the rules only ask whether they are there)
    pinned = {a.buf for a in list(plan.head_outs) + list(plan.feats)}
    L.assign_amax(plan.ops)
    assert L.link_pools(L.BufferIndex(plan.ops), L.has_f16) == 2
    assert L.link_maxpools(L.BufferIndex(plan.ops), pinned, L.has_f16) == 1
    index = L.BufferIndex(plan.ops)
    for _, cons in L.split_pairs(index, plan.buffers, pinned, L.has_f16):
        for c in cons:
            c['gp_in'] = True
    tabs = [json.load(open(_TUNED_PATHS[m])) for m in ('f16x2', 'bf16x3')]
    L.apply_tuned(plan.ops, *tabs)
    assert all(op['cfg'] >= 0 for op in plan.ops if op['op'] in ('conv', 'dcn'))          # the table knows every layer of its workload
    links, fused, _ = L.decide_links(plan.ops, index, plan.buffers, pinned, L.has_f16, K.conv_cfg)
    linked = [c for _, cons in links for c in cons]
    assert (len(linked), len(fused)) == (39, 2) and len(set(linked)) == len(linked)
    assert all(a in linked for a, _ in fused)
