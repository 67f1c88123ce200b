"""What the training step decides without a device -- table keys, tile ids, the forward form of a convolution unit, the flat
parameter layout and its all-reduce buckets, the detection block's schedule, the PPYOLO_HIP_TRAIN_* switches -- as pure
functions (tests/test_train_host_logic.py, tests/test_train_cfg_ids.py).  train.py owns the state and issues the launches;
nothing here imports torch, loads the library or calls an op: the `cfg id -> ConvCfg` lookup (ops.conv_cfg) and the descriptor
list (ops.conv_cfgs) are handed in, as plan_links takes `cfg_of`."""
import collections


def r32(c):
    return (c + 31) // 32 * 32


def shape_key(op, N, H, W, C, K, R, stride, f=False, p=False, g=False):
    """Shape key of a launch in the measured (tile config, split-K) tables: the geometry the forward kernel sees.  op: 'conv', or
    'dcnf' (ids of the fused DCNv2 kernel).  ':f': f16x2 operands at hand; ':p' / ':g': plan_links.tune_key."""
    return '%s:N%d:H%d:W%d:C%d:K%d:R%d:s%d%s%s%s' % (op, N, H, W, C, K, R, stride, ':f' if f else '', ':p' if p else '', ':g' if g else '')


def dgrad_key(N, Ho, Wo, Kout, C, R):
    """(key, chunks) of a stride-1 data gradient: the forward kernel on the transposed geometry -- C' = K rounded up to 32, K' = C."""
    return shape_key('conv', N, Ho, Wo, r32(Kout), C, R, 1), R * R * r32(Kout) // 32


def train_fwd_cfg(cfg_id, splitk, cfg_of):
    """(tile configuration, split-K) a table names for a forward convolution -> the pair the training forward launches.  The
    training tables fall back on the inference tables' entries, whose ids include families that cannot give the BatchNorm
    statistics this forward takes from the epilogue:
      * a k-parity tile (round 6): the same tile with one consumer group (its stats_twin), split-K kept;
      * a wave-private small-output tile: its split-K counts k-parts inside the workgroup, not workspace splits, and it writes no
        statistics -- the library's own choice instead, (-1, 0).
    Data gradients keep the table's ids: they take no statistics, and every family runs them (tests/test_gpu_train_replay.py)."""
    d = cfg_of(cfg_id) if cfg_id >= 0 else None
    if d is not None and d.family == 'kparity':
        return d.stats_twin, splitk
    if d is not None and d.splitk_mode == 'workgroup':
        return -1, 0
    return cfg_id, splitk


def tune_cfgs(f16, cfgs):
    """The tile configurations a training forward is measured on: the nine bf16x3 tiles; with the f16x2 operands the f16x2 tiles x
    {2, 3, 4} LDS stages and the specialised-wave tiles that emit the BatchNorm statistics it takes from the epilogue (no k-parity tile)."""
    fams = ('f16x2', 'ws', 'ws_pre') if f16 else ('bf16x3',)
    return [d.id for d in cfgs if d.family in fams and d.bn_stats == f16]


Switches = collections.namedtuple('Switches', 'wgrad_side async_tail bn_epilogue bn_epilogue_all f16 fp32 overlap fuse_stats prefetch')


def switches(environ, world_size, nccl, external):
    """The PPYOLO_HIP_TRAIN_* variables TrainStep.__init__ reads, resolved; nccl: the process group's backend is nccl (= RCCL).
      wgrad_side (.._WGRAD_STREAM, default 1): the weight gradient of a head convolution has no consumer before the optimizer: it runs
        on a SECOND stream beside the data gradient chain (its own workspace; the operands are kept alive until the join at the end
        of the backward).  Same kernels, same results bit for bit; 0 puts it back in line.
      async_tail (.._ASYNC_TAIL, default 1): ... and so do the optimizer step, the EMA update and the re-split of the updated weights
        (sgd, _prepare_weights): the next step's frozen layers do not read a trainable parameter, so its forward starts while they
        run; the first use of a trainable parameter (weight() / param()) or a reader outside the step (sync_to_model, grads) waits
        for them (_await_params).  It runs on that second stream, so it needs wgrad_side.  0: in line.
      bn_epilogue, bn_epilogue_all (.._BN_EPILOGUE): frozen 1x1 layers on the streaming kernel, BatchNorm from the convolution's own
        epilogue, no raw tensor (conv_form).  0 = off, 1 = the layers the table puts on the streaming kernel, 2 (default) = those and
        every frozen C = 128 1x1 layer the kernel accepts, whatever tile the table names: 11.82 -> 11.58 -> 11.48 ms on the R50vd-608 step.
      f16, fp32 (.._MATH): f16x2 (default) = forward convolutions on the f16x2 kernels (3 MFMA products instead of 6) where the input's
        maximum is tracked -- by bn_train_apply for every normalised activation, propagated through concatenations / pooling /
        DropBlock; bf16x3 keeps every convolution on the exact bf16 split; fp32 (bench.py's value_fp32_exact leg; with PPY_WGRAD_FP32=1
        and PPY_DGRAD_FP32=1 in the environment of the process): every convolution, data gradient and weight gradient on the
        exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
      overlap (.._OVERLAP): gradient buckets go out as asynchronous all-reduces DURING the backward.  With backend nccl that puts
        RCCL's fp32 sum kernels beside this library's 16-bit-MFMA kernels on the same CUs -- the co-residence under which a
        packed-fp32 instruction form misreads.  librccl's gfx950 code holds 945 v_pk_*_f32, none in that form
        (tools/rccl_pk_scan.py -> profiles/r03_rccl_pk_scan.txt), but the pair has never executed on hardware (no multi-GPU box):
        under nccl with several ranks the overlap is therefore OPT-IN (=1) and the default is one collective after the backward, when
        no MFMA kernel of this rank is in flight; other backends (gloo: host reductions) overlap unless =0.  Off with an external
        optimizer, whatever the variable says.
      fuse_stats (.._FUSE_STATS, default 1): BatchNorm statistics from the conv epilogue.
      prefetch (.._PREFETCH, default 1): with the whole backbone frozen (freeze_at = 5, the reference's configurations) its
        training-mode forward reads no trainable parameter, so the NEXT batch's backbone can run on a third stream beside THIS
        batch's head forward / loss / backward (prefetch_backbone, step(..., next_x=...)): same kernels on the same inputs in the
        same order per tensor -- bit-identical losses, gradients and running statistics -- with its own workspace, BatchNorm
        partials and (two alternating) blocks of tracked-maximum slots.  0 ignores next_x."""
    get = environ.get
    wgrad_side = get('PPYOLO_HIP_TRAIN_WGRAD_STREAM', '1') == '1'
    epi, math, ov = get('PPYOLO_HIP_TRAIN_BN_EPILOGUE', '2'), get('PPYOLO_HIP_TRAIN_MATH', 'f16x2'), get('PPYOLO_HIP_TRAIN_OVERLAP')
    return Switches(wgrad_side=wgrad_side, async_tail=wgrad_side and get('PPYOLO_HIP_TRAIN_ASYNC_TAIL', '1') == '1',
                    bn_epilogue=epi in ('1', '2'), bn_epilogue_all=epi == '2', f16=math == 'f16x2', fp32=math == 'fp32',
                    overlap=((ov == '1') if (nccl and world_size > 1) else (ov != '0')) and not external,
                    fuse_stats=get('PPYOLO_HIP_TRAIN_FUSE_STATS', '1') == '1', prefetch=get('PPYOLO_HIP_TRAIN_PREFETCH', '1') == '1')


def conv_form(has_bn, f16, trainable, coord, R, S, stride, C, Kout, HW, table, sw, cfg_of, stream_first):
    """How a convolution unit's forward runs -> (form, cfg, splitk).  f16: the f16x2 operands are at hand; coord: behind a CoordConv;
    C: padded input channels; HW: input pixels per image; table: the tables' (cfg, splitk); sw: Switches; stream_first: the
    streaming kernel's first id.  Forms:
      'epilogue': frozen 1x1 layers on the streaming kernel (the HBM-bound conv3 / shortcut layers of stage 2): the raw output is
                  never stored -- one launch for the statistics, one that applies the BatchNorm to its own accumulators;
      'stats':    the convolution with the BatchNorm statistics from its epilogue (the f16x2 kernels, one split): saves the
                  statistics kernel's pass over the raw output;
      'plain':    the convolution, then (with BatchNorm) the separate statistics pass."""
    cfg, splitk = (-1, 0) if sw.fp32 else train_fwd_cfg(table[0], table[1], cfg_of)
    fused = has_bn and f16 and sw.fuse_stats
    streams = fused and not trainable and not coord and (R, S, stride) == (1, 1, 1)
    if sw.bn_epilogue and streams and splitk == 1 and cfg >= 0 and cfg_of(cfg).family == 'stream':
        return 'epilogue', cfg, splitk
    # PPYOLO_HIP_TRAIN_BN_EPILOGUE=2: every frozen C = 128 1x1 layer the kernel accepts, whatever tile the table names (measured +0.8 %)
    groups = Kout // 128
    if sw.bn_epilogue_all and streams and C == 128 and Kout % 128 == 0 and groups & (groups - 1) == 0 and groups <= 16 and HW >= 32:
        return 'epilogue', stream_first, 1
    if fused and splitk == 1 and cfg >= 0 and cfg_of(cfg).bn_stats:
        return 'stats', cfg, splitk
    return 'plain', cfg, splitk


NORMS = ('bn', 'gn', 'af')                 # the state_dict's sub-module names: BatchNorm2d, GroupNorm, AffineChannel
GN_MAX_CHANNELS = 2048                     # ppy_group_norm_f32 / _bwd_f32: PPY_ERR_UNSUPPORTED above


def norm_of(keys, prefix):
    """Which norm a Conv2dUnit holds, read from its state_dict keys ('<prefix>.bn.weight' ...): 'bn' / 'gn' / 'af' / None."""
    for n in NORMS:
        if '%s.%s.weight' % (prefix, n) in keys:
            return n
    return None


def norm_form(norm, act, trainable):
    """How the training forward and backward of a unit run behind its convolution, beside conv_form (which keeps deciding how the
    convolution of a 'bn' unit runs).  norm: norm_of(); act: None / 'relu' / 'leaky' / 'mish'; trainable: its parameters train.
      'none':         no norm: the convolution with its bias (the output convolutions);
      'bn':           BatchNorm on batch statistics + relu / leaky / nothing: train.hip, exactly as before;
      'bn_mish':      BatchNorm with act = None, then Mish in place; backward: Mish backward (pre-activation recomputed from the raw
                      output and the batch scale / shift), then the BatchNorm backward with act = None;
      'gn':           raw convolution (scale 1, shift = conv bias), GroupNorm training forward (any activation, the residual inside);
                      backward: GroupNorm backward, then the convolution's weight / data gradients;
      'af_fold':      frozen AffineChannel: (af.weight, af.bias + conv_bias * af.weight) and the activation in the convolution's own
                      epilogue, no extra launch -- the inference path's fold;
      'af_fold_mish': ... Mish cannot go into the epilogue: it follows as a launch;
      'af_train':     trainable AffineChannel: raw convolution, one apply launch (any activation), the AffineChannel backward."""
    if act not in (None, 'relu', 'leaky', 'mish'):
        raise ValueError('activation %r' % (act,))
    if norm is None:
        if act == 'mish':
            raise ValueError('Mish behind a convolution without a norm is not implemented in the training step')
        return 'none'
    if norm == 'bn':
        return 'bn_mish' if act == 'mish' else 'bn'
    if norm == 'gn':
        return 'gn'
    if norm == 'af':
        return 'af_train' if trainable else ('af_fold_mish' if act == 'mish' else 'af_fold')
    raise ValueError('norm %r' % (norm,))


def norm_refusal(name, norm, channels, groups, norm_decay):
    """Why the training step refuses a GroupNorm / AffineChannel unit, by its name -- or None."""
    if norm not in ('gn', 'af'):
        return None
    if norm == 'gn' and (groups <= 0 or channels % groups != 0):
        return '%s: GroupNorm of %d channels in %d groups (C %% groups != 0)' % (name, channels, groups)
    if norm == 'gn' and channels > GN_MAX_CHANNELS:
        return '%s: GroupNorm of %d channels: the kernels implement C <= %d' % (name, channels, GN_MAX_CHANNELS)
    if float(norm_decay) != 0.0:
        return ('%s: norm_decay = %r: norm scales / offsets are stepped without weight decay (every configuration has 0)'
                % (name, norm_decay))
    return None


def kernel_shape(shape):
    """A parameter's shape in kernel layout: a convolution weight [K, C, R, S] is kept KRSC with C padded to a multiple of 32 (the
    stem's 3 channels, a CoordConv's C + 2); everything else as the state_dict has it."""
    return (shape[0], shape[2], shape[3], r32(shape[1])) if len(shape) == 4 else tuple(shape)


def flat_layout(keyed_shapes):
    """[(key, kernel-layout shape)] of the trainable tensors, in state_dict order -> ({key: (offset, numel, shape)}, total, n_decay).
    Convolution weights first, then the conv_offset biases (the reference decays them like a weight: custom_layers.py:189-194) --
    [0, n_decay) is the weight-decay group -- then biases and the scales / offsets of BatchNorm, GroupNorm and AffineChannel
    ('.bn.' / '.gn.' / '.af.' + 'weight' / 'bias': no decay, reference custom_layers.py:216-241); every tensor padded to 64 floats."""
    convs = [(k, s) for k, s in keyed_shapes if len(s) == 4] + [(k, s) for k, s in keyed_shapes if k.endswith('.conv_offset.bias')]
    rest = [(k, s) for k, s in keyed_shapes if len(s) != 4 and not k.endswith('.conv_offset.bias')]
    offs, total, n_decay = {}, 0, 0
    for i, (k, shp) in enumerate(convs + rest):
        n = 1
        for d in shp:
            n *= d
        offs[k] = (total, n, tuple(shp))
        total += (n + 63) // 64 * 64
        if i == len(convs) - 1:
            n_decay = total
    return offs, total, n_decay


def stage_of(key):
    """Backbone stage (1..5) a state_dict key belongs to; 6 = the head."""
    return int(key[len('backbone.stage')]) if key.startswith('backbone.stage') else 6


def bucket_of(key):
    """Gradient bucket of a parameter: a detection block, the head's output / transition convolutions, a backbone stage --
    the units in which the backward finishes its gradients (last layers first)."""
    q = key.split('.')
    if q[0] == 'backbone':
        return q[1][:6]                      # 'stage5'
    return '.'.join(q[:3]) if q[1] == 'detection_blocks' else 'head.tail'


def unit_of(key):
    """The Conv2dUnit prefix a parameter key belongs to ('....conv.weight' / '.bn.bias' / '.conv.conv_offset.bias' ...)."""
    for tail in ('.conv.conv_offset.weight', '.conv.conv_offset.bias', '.conv.dcn_weight', '.conv.weight', '.conv.bias', '.bn.weight',
                 '.bn.bias', '.gn.weight', '.gn.bias', '.af.weight', '.af.bias'):
        if key.endswith(tail):
            return key[:-len(tail)]
    return key


def buckets(keys, layout, total):
    """{bucket: {'units': the units whose gradients it holds, 'ranges': [(start, end) of the flat buffer]}}, buckets in the order
    `keys` meets them: the keys of a bucket are (nearly) contiguous in both parameter groups, so a bucket is two or three ranges."""
    spans, out = {}, {}
    for k in keys:
        o, n, _ = layout[k]
        spans.setdefault(bucket_of(k), []).append((o, o + (n + 63) // 64 * 64))
        out.setdefault(bucket_of(k), dict(units=set(), ranges=[]))['units'].add(unit_of(k))
    for b, iv in spans.items():
        iv.sort()
        merged = [list(iv[0])]
        for a, e in iv[1:]:
            if a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e)
            else:
                merged.append([a, e])
        out[b]['ranges'] = [(a, min(e, total)) for a, e in merged]
    return out


Step = collections.namedtuple('Step', 'kind n coord dest')


def detection_schedule(hcfg, is_first):
    """DetectionBlock.__call__ (reference model/head.py:146-231) as ordered steps; n = the module's index in `layers` (the
    state_dict's `layers.N`; in `tip_layers` for the tip).  kind: 'conv'; 'spp' (the pooled copies beside a convolution produced with
    dest 'spp' = into slot 0 of a four times as wide buffer); 'drop' (every DropBlock module, active or not); 'route' and 'tip' (the
    block's two results).  coord: the convolution sits behind a CoordConv; dest 'coord': the tensor's one consumer is a CoordConv,
    so it is produced into that layer's coordinate-ready buffer."""
    nblk, coord = hcfg.get('conv_block_num', 2), hcfg.get('coord_conv', True)
    use_spp, drop, active = hcfg.get('spp', True), hcfg.get('drop_block', True), hcfg.get('drop_active', True)
    to_coord = 'coord' if coord else None
    steps, n = [], 0                       # n: the next module's index (a CoordConv module in front of every coord-able convolution)
    for j in range(nblk):
        # (an active DropBlock behind this pair takes the coordinate-ready buffer instead of the pair's last convolution)
        drops = drop and ((j == 0 and not is_first) or (j == nblk - 1 and is_first))
        last_dest = None if (drops and active) else to_coord
        if use_spp and is_first and j == 1:
            steps += [Step('conv', n + 1, coord, 'spp'), Step('spp', n + 2, False, None), Step('conv', n + 3, False, None),
                      Step('conv', n + 4, False, last_dest)]
            n += 5
        else:
            steps += [Step('conv', n + 1, coord, None), Step('conv', n + 2, False, last_dest)]
            n += 3
        if drop and j == 0 and not is_first:
            steps.append(Step('drop', n, False, to_coord))
            n += 1
    if drop and is_first:
        steps.append(Step('drop', n, False, to_coord))
        n += 1
    return steps + [Step('route', n + 1, coord, to_coord), Step('tip', 1, coord, None)]
