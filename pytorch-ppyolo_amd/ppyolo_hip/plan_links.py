"""Which ops of a plan share a launch, and what follows from it -- pure plan logic, no device (tests/test_plan_host_logic.py).

HipExecutor derives the link state in ONE order: assign_amax; link_pools, then link_maxpools (structural links);
split_pairs marks the 'gp_in' candidates; apply_tuned; decide_links -- pre-split links and fused pairs, from the tile ids the table
chose; sync_plan over the final state.  Whatever changes a tile id afterwards repeats the last two (HipExecutor._link_splits).
op_io(op) is what an op reads and writes UNDER the links made so far and a BufferIndex a snapshot of it: whoever makes links
builds a new one before the next rule reads it.  A `cfg id -> ConvCfg` lookup is handed in (ops.conv_cfg; a table in a test)."""
from ._lib import PPYoloHipError
from .train_plan import shape_key


def has_f16(op):
    """f16x2 operands at hand: split fp16 weights and a tracked input maximum (the executor's predicate for every rule below)."""
    return op.get('wf16') is not None and op.get('amax_in_id') is not None


def tune_key(op, with_g=True):
    """Shape key of a conv / DCN launch in the measured (tile config, split-K) table.  Launches that can use the
    f16x2 kernels (split fp16 weights at hand, tracked input maximum) carry ':f' -- the same shape without them
    (CoordConv layers, stem side) needs its own entry."""
    x = op['x']
    Kout, R, S, C = op['w'].shape
    # ('dcnf': ids of the fused DCNv2 kernel, ops.dcnv2_num_configs -- not the convolution's numbering)
    # ':p': the layer also owns the 2x2 average of its output (link_pools)
    # ':g': the layer's input can arrive pre-split from its one producer (split_pairs marks 'gp_in'): its main loop has
    # no split work, another tile may win -- such entries are measured in that form; without one the plain entry is used
    return shape_key('dcnf' if op['op'] == 'dcn' else op['op'], x.N, x.H, x.W, C, Kout, R, op['stride'], has_f16(op),
                     op.get('pool') is not None, bool(op.get('gp_in') and with_g))


def apply_tuned(ops, tab, tab_x3):
    """The measured table's (tile id, split-K) for every conv / DCN op that has none yet (cfg < 0); tab_x3: the bf16x3 table, which
    a layer without ':f' in f16x2 mode behaves by.  Needs 'pool' and 'gp_in' marked: both are part of the key."""
    for op in ops:
        if op['op'] in ('conv', 'dcn') and op['cfg'] < 0:
            ent = tab.get(tune_key(op)) or tab.get(tune_key(op, False)) or tab_x3.get(tune_key(op, False))
            if not ent and op.get('pool') is not None:                   # no entry for the pooled form: the plain shape's
                k0 = tune_key(dict(op, pool=None), False)
                ent = tab.get(k0) or tab_x3.get(k0)
            if ent:
                op['cfg'], op['splitk'] = ent[:2]


def op_io(op):
    """(input buffer ids, output buffer ids) of a plan op."""
    t = op['op']
    if t == 'conv' and op.get('b2b_of') is not None:         # computed inside the launch of the convolution in front of it (b2b_pairs)
        return [], []
    if t == 'conv' and op.get('b2b') is not None:
        b = op['b2b']
        return [op['x'].buf, b['res'].buf], [b['y'].buf] + ([b['pool'].buf] if b.get('pool') is not None else [])
    if t == 'conv':
        ins = [op['x'].buf] + ([op['res'].buf] if op['res'] is not None else [])
        if op.get('mpool') is not None:          # only the pooled tensor is written (link_maxpools)
            return ins, [op['mpool'].buf]
        return ins, [op['y'].buf] + ([op['pool'].buf] if op.get('pool') is not None else [])
    if t == 'stem':
        return [], [op['y'].buf]
    if t in ('avgpool', 'maxpool') and op.get('owner') is not None:      # written by its producer's launch (link_pools / link_maxpools)
        return [], []
    if t in ('maxpool', 'avgpool'):
        return [op['x'].buf], [op['y'].buf]
    if t == 'spp':
        return [op['x'].buf], [op['y5'].buf]
    if t == 'dcn':
        return [op['x'].buf, op['om'].buf], [op['y'].buf]
    if t == 'gn':
        return [op['x'].buf] + ([op['res'].buf] if op['res'] is not None else []), [op['y'].buf]
    if t == 'mish':          # in place: a second writer of its buffer, which keeps every link rule off the convolution in front of it
        return [op['x'].buf], [op['x'].buf]
    raise PPYoloHipError('unknown plan op %r' % t)


class BufferIndex(object):
    """buffer id -> [(position, op)] in plan order, for the readers and for the writers of the buffer: op_io of every op, once."""
    def __init__(self, ops):
        self.ops, self.readers, self.writers = ops, {}, {}
        for i, op in enumerate(ops):
            ins, outs = op_io(op)
            for b in ins:
                self.readers.setdefault(b, []).append((i, op))
            for b in outs:
                self.writers.setdefault(b, []).append((i, op))


def assign_amax(ops):
    """Blocks of tracked per-image maxima for the f16x2 kernels: sets op['amax_out_id'] / ['amax_in_id'] / ['amax_in2_id'],
    returns the number of blocks.  A conv / DCN launch merges max|y| into the block of its output BUFFER (the writers of a concat
    buffer share one); a pooled tensor inherits the block of its input (max- and average-pooling never exceed it; SPP writes into
    its own input buffer; the DCN columns are bounded by the DCN input); the stem kernel tracks its output as well.  Round 6: when
    a convolution writes into a buffer that so far only holds a pooled tensor -- the folded projection shortcut's wide buffer
    [conv2 output | pooled block input] -- the buffer gets a block of its OWN for what convolutions write and keeps the inherited
    one as a second, read-only block ('amax_in2_id' of its readers): the block input's other readers (the head's C3 / C4
    convolutions) no longer see conv2's maximum (round-5 advisor).  Only ppy_conv2d_bn_act_split_f32 takes the
    second block: link_pools, link_maxpools and b2b_pairs leave a convolution that carries 'amax_in2_id' a launch of its own.
    GroupNorm and Mish: ppy_group_norm_f32 tracks nothing, so the buffer a 'gn' op writes into has NO block, whoever else writes into
    it (a concat buffer shared with convolutions included) -- its readers get amax_in_id None, has_f16 is false for them and they run
    on the non-f16x2 tiles.  |mish(x)| <= |x|, so a 'mish' op (in place) keeps its buffer's block, as pooling does: the maximum the
    convolution in front of it tracked still bounds what the readers see."""
    amax_of, aux_of, inherited, untracked, nblocks = {}, {}, set(), set(), 0
    for op in ops:
        t = op['op']
        if t == 'gn':
            b = op['y'].buf
            untracked.add(b)
            inherited.discard(b)
            amax_of.pop(b, None)
            aux_of.pop(b, None)
        elif t in ('conv', 'dcn') and op['y'].buf in untracked:
            op['amax_out_id'] = None
            op['amax_in_id'] = amax_of.get(op['x'].buf)
            op['amax_in2_id'] = aux_of.get(op['x'].buf)
        elif t in ('conv', 'dcn'):
            b = op['y'].buf
            if b in inherited:
                inherited.discard(b)
                aux_of[b] = amax_of.pop(b)
            if b not in amax_of:
                amax_of[b] = nblocks
                nblocks += 1
            op['amax_out_id'] = amax_of[b]
            op['amax_in_id'] = amax_of.get(op['x'].buf)
            op['amax_in2_id'] = aux_of.get(op['x'].buf)
        elif t in ('maxpool', 'avgpool'):
            src = amax_of.get(op['x'].buf)
            if src is not None and op['y'].buf not in untracked:
                yb = op['y'].buf
                if yb in amax_of and yb not in inherited:      # a convolution wrote into this buffer first: second block
                    aux_of[yb] = src
                else:
                    amax_of[yb] = src
                    inherited.add(yb)
        elif t == 'stem':
            amax_of[op['y'].buf] = nblocks
            op['amax_out_id'] = nblocks
            nblocks += 1
    return nblocks


def link_pools(index, has_f16, two_streams=False):
    """The vd shortcut's AvgPool2d(2, 2) (reference model/resnet_vd.py:29-33) belongs to the launch that produces its input: gives
    every 'avgpool' op whose input slice is written by exactly one 1x1 / stride-1 convolution that ppy_conv1x1_expand_f32 accepts
    (C = 64 with K % 64 == 0, or C = 128 with K % 128 == 0; K / 64 resp. K / 128 a power of two <= 16; no upsampling, no position
    bias, one tracked-maximum block; has_f16(op): f16x2 operands at hand) to that convolution: conv['pool'] = the pooled slice,
    avgpool['owner'] = the convolution.  The producer then writes the 2x2 average from its own epilogue (cfg = a streaming id,
    csrc/conv_stream.hip) or, on any other tile, the pooling launch follows it immediately; the 'avgpool' op is skipped either
    way.  Returns the number of links."""
    n = 0
    for i, op in enumerate(index.ops):
        if op['op'] != 'avgpool':
            continue
        x = op['x']
        # (a route buffer has several writers, each of its own channel slice: the producer is the EARLIER one that writes x's)
        prods = [o for j, o in index.writers.get(x.buf, []) if j < i and (o['op'] != 'conv' or (o['y'].coff < x.coff + x.C
                                                                                                 and x.coff < o['y'].coff + o['y'].C))]
        if len(prods) != 1 or prods[0]['op'] != 'conv':
            continue
        c = prods[0]
        Kout, R, S, C = c['w'].shape
        y = c['y']
        groups = Kout // 64 if C == 64 else Kout // 128           # (what ppy_conv1x1_expand_f32 accepts)
        if (R, S, c['stride']) != (1, 1, 1) or C not in (64, 128) or Kout % (64 if C == 64 else 128) or groups & (groups - 1) \
                or groups > 16 or c['ups'] or c['posb'] is not None or not has_f16(c) or c.get('amax_in2_id') is not None \
                or (two_streams and c.get('stream', 0) != op.get('stream', 0)) \
                or (y.buf, y.coff, y.C) != (x.buf, x.coff, x.C) or x.H % 2 or x.W % 2 or x.H * x.W < 32:
            continue
        c['pool'] = op['y']
        op['owner'] = c
        n += 1
    return n


def link_maxpools(index, pinned, has_f16):
    """The stem's MaxPool2d(3, 2, 1) (reference model/resnet_vd.py:103, 136) belongs to the launch of the convolution in front of it
    (csrc/conv_patch.hip, MPOOL): a 'maxpool' op whose input is the WHOLE buffer written by one convolution that
    ppy_conv3x3_maxpool_f32 accepts (3x3 / stride 1 / pad 1, C = 32 -> K = 64, no shortcut / upsampling / position bias, one
    tracked-maximum block; has_f16(op): f16x2 operands at hand) and read by nothing else: conv['mpool'] = the pooled slice,
    maxpool['owner'] = the convolution, whose launch then writes ONLY the pooled tensor -- the 304 x 304 x 64 tensor between them is
    neither written nor read.  Returns the number of links."""
    n = 0
    for op in index.ops:
        if op['op'] != 'maxpool':
            continue
        x = op['x']
        prods = [o for _, o in index.writers.get(x.buf, [])]
        readers = [o for _, o in index.readers.get(x.buf, []) if o is not op]
        if len(prods) != 1 or prods[0]['op'] != 'conv' or readers or x.buf in pinned:
            continue
        c = prods[0]
        Kout, R, S, C = c['w'].shape
        y = c['y']
        if (R, S, c['stride'], c['pad'], C, Kout) != (3, 3, 1, 1, 32, 64) or c['ups'] or c['posb'] is not None or c['res'] is not None \
                or c.get('pool') is not None or not has_f16(c) or c.get('stream', 0) != op.get('stream', 0) \
                or c.get('amax_in2_id') is not None or (y.buf, y.coff, y.C) != (x.buf, x.coff, x.C) or x.coff != 0:
            continue
        c['mpool'] = op['y']
        op['owner'] = c
        n += 1
    return n


def split_pairs(index, buffers, pinned, has_f16, only_3x3=False):
    """[(producer, [consumers])] between which a tensor may travel PRE-SPLIT, whatever tiles they run on -- a
    buffer written by ONE convolution (the whole buffer, no shortcut term, no upsampled store, no pooled twin, a multiple of 32
    channels) and read ONLY by convolutions, as their input: a bottleneck's conv1 -> conv2, the head's 1x1 -> 3x3 -> 1x1 chains,
    and a route with its two readers (the tip 3x3 and the 1x1 in front of the upsampling).  pinned: buffers that something
    outside the convolution chain reads (feature maps, head outputs).  has_f16(op): f16x2 operands at hand.  only_3x3: A/B switch
    -- 1x1 consumers gain less (they split every activation once per wave column, a 3x3 nine times) but they gain: R50vd-608 bs 8
    +0.9 % on top of the 3x3 links."""
    pairs = []
    for b, ws_ in index.writers.items():
        if len(ws_) != 1 or b in pinned:
            continue
        pr = ws_[0][1]
        ld = buffers[b][3]
        y = pr.get('y')
        if pr['op'] != 'conv' or not has_f16(pr) or pr['ups'] or pr['res'] is not None or pr.get('pool') is not None \
                or y.buf != b or y.coff != 0 or y.C != ld or ld % 32:
            continue
        cons = [c for _, c in index.readers.get(b, [])]
        ok = bool(cons)
        for c in cons:
            x = c.get('x')
            if c['op'] != 'conv' or not has_f16(c) or x is None or x.buf != b or x.coff != 0 or x.C != ld \
                    or (c['res'] is not None and c['res'].buf == b) or (only_3x3 and c['w'].shape[1] != 3):
                ok = False
        if ok and len(set(id(c) for c in cons)) == len(cons):
            pairs.append((pr, cons))
    return pairs


def b2b_pairs(index, buffers, pinned, has_f16):
    """[(conv A, conv B)] that ppy_conv3x3_conv1x1_f32 can run as ONE launch (round 5, csrc/conv_b2b.hip: the 64-channel tensor
    between them is neither written nor read) -- conv2 -> conv3 of an identity bottleneck (reference model/resnet_vd.py:81-87): A =
    3x3 / stride 1 / pad 1, 64 -> 64, ReLU, no shortcut / position bias / upsampling, writing a whole buffer that ONLY B reads; B =
    1x1 / stride 1, 64 -> 256, ReLU, with a shortcut, no position bias / upsampling; one tracked-maximum block each."""
    out = []
    for a in index.ops:
        if a['op'] != 'conv' or not has_f16(a) or a.get('amax_in2_id') is not None:
            continue
        Ka, R, S, Ca = a['w'].shape
        y = a['y']
        if (R, S, a['stride'], a['pad'], Ca, Ka, a['act']) != (3, 3, 1, 1, 64, 64, 'relu') or a['res'] is not None or a['posb'] is not None \
                or a['ups'] or a.get('pool') is not None or a.get('mpool') is not None or y.buf in pinned \
                or y.coff != 0 or y.C != buffers[y.buf][3] or len(index.writers.get(y.buf, [])) != 1:
            continue
        rd = index.readers.get(y.buf, [])
        if len(rd) != 1 or rd[0][1]['op'] != 'conv':
            continue
        b = rd[0][1]
        Kb, Rb, Sb, Cb = b['w'].shape
        x = b['x']
        if (Rb, Sb, b['stride'], b['pad'], Cb, Kb, b['act']) != (1, 1, 1, 0, 64, 256, 'relu') or b['res'] is None or b['posb'] is not None \
                or b['ups'] or not has_f16(b) or (x.buf, x.coff, x.C) != (y.buf, 0, 64) or b['res'].buf == y.buf \
                or b.get('stream', 0) != a.get('stream', 0) or b.get('amax_in2_id') is not None:
            continue
        out.append((a, b))
    return out


def static_bound(op, posb_absmax=None):
    """(mul, add) with max|y| <= mul * max|x| + add for a convolution's output, in float64 and rounded up: per output channel |scale|
    * sum|w|, and |shift| plus |scale| * posb_absmax (per-channel maximum of the CoordConv bias map, where the op has one).  A
    producer scales its pre-split output by it, and a fused pair the tensor between its two convolutions, without a second pass."""
    w, sc, sh = op['w'], op['scale'], op['shift']
    l1 = w.abs().double().sum(dim=(1, 2, 3))
    mul = float((sc.abs().double() * l1).max())
    add = sh.abs().double()
    if posb_absmax is not None:
        add = add + posb_absmax * sc.abs().double()
    return mul * (1.0 + 2.0 ** -8), float(add.max()) * (1.0 + 2.0 ** -8) + 1e-30


def split_leaves_launch(op, cfg_of):
    """Does this op's split-K go through partial sums in memory (a second launch combines them)?  Then it reads and writes plain fp32."""
    return op.get('splitk', 0) > 1 and not (op['op'] == 'conv' and op.get('cfg', -1) >= 0 and cfg_of(op['cfg']).splitk_mode == 'workgroup')


def split_capable(cfg, consumer, cfg_of):
    """Does this tile configuration read (consumer) / write pre-split tensors?"""
    return cfg >= 0 and (cfg_of(cfg).reads_presplit if consumer else cfg_of(cfg).writes_presplit)


def takes_presplit(op, cfg_of, consumer=True):
    """Would this op, as it stands (cfg, splitk), read its input (consumer) / write its output pre-split?  (A 'gp_in' layer is measured so.)"""
    return not split_leaves_launch(op, cfg_of) and split_capable(op['cfg'], consumer, cfg_of)


def decide_links(ops, index, buffers, pinned, has_f16, cfg_of, presplit=True, only_3x3=False, b2b=True, rejected=()):
    """Which structurally possible links the tiles at hand (op['cfg'], op['splitk']) allow.  `index`: of the plan with NO pair fused.
    Returns (links, fused, rounds), all in op positions: links = [(producer, [consumers])] between which the tensor travels
    pre-split ("global pre-split", DESIGN.md 4.1g: the producer stores its output as the consumers' finished MFMA operands, two
    fp16 terms of y * s_image, same bytes per pixel, and their main loops carry no scale / split work) -- the producer's tile
    writes that form, every consumer's reads it, no split-K of theirs leaves the launch, and every reader takes the tensor so or
    none does; fused = [(a, b)] of b2b_pairs that run as one launch.  A fused pair needs its input pre-split (csrc/conv_b2b.hip
    reads finished operands) and its stand-alone form may allow other links, so: derive the links with every pair fused that is
    not in `rejected`; reject the pairs whose first convolution got no link -- only those, not every pair; again, until none is
    rejected (rounds: the derivations that took).  presplit / only_3x3 / b2b: PPYOLO_HIP_PRESPLIT, .._PRESPLIT_3X3_ONLY, .._B2B."""
    pos = {id(op): i for i, op in enumerate(ops)}
    cand = [(pos[id(a)], pos[id(b)]) for a, b in b2b_pairs(index, buffers, pinned, has_f16)] if b2b else []
    struct = [(pos[id(pr)], [pos[id(c)] for c in cons]) for pr, cons in split_pairs(index, buffers, pinned, has_f16, only_3x3)] if presplit else []
    rejected, rounds = set(rejected), 0
    while True:
        rounds += 1
        fused = [(a, b) for a, b in cand if a not in rejected]
        first = {a for a, _ in fused}
        # (the tensor behind a fused first convolution is never written; a fused first convolution reads pre-split whatever its cfg)
        links = [(pr, cons) for pr, cons in struct if pr not in first and takes_presplit(ops[pr], cfg_of, False)
                 and all(c in first or takes_presplit(ops[c], cfg_of) for c in cons)]
        undone = first - {c for _, cons in links for c in cons}
        if not undone:
            return links, fused, rounds
        rejected |= undone


def sync_plan(ops, multi_stream):
    """Cross-stream dependencies under the CURRENT links, (waits, needs_event, side_tail): waits[i] = the earlier writers, on the
    other stream, of a buffer op i reads (buffers are never reused, concat buffers have several writers of disjoint slices ->
    wait for all of them); needs_event = the ops somebody waits for; side_tail = the last op of the side stream, joined before
    decode / the end of the step.  A fused pair launches as its FIRST convolution: that one waits for the shortcut's writer."""
    writers, waits, needs_event = {}, [[] for _ in ops], set()
    for i, op in enumerate(ops):
        ins, outs = op_io(op)
        s = op.get('stream', 0) if multi_stream else 0
        for bid in ins:
            for j in writers.get(bid, []):
                sj = ops[j].get('stream', 0) if multi_stream else 0
                if sj != s and j not in waits[i]:
                    waits[i].append(j)
                    needs_event.add(j)
        for bid in outs:
            writers.setdefault(bid, []).append(i)
    side_tail = max([i for i, op in enumerate(ops) if op.get('stream', 0)], default=None) if multi_stream else None
    return waits, needs_event, side_tail
