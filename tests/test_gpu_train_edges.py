"""The launch-level float64 checkers of tests/launch_replay.py, with their own bounds, on the edge table of tests/train_edge_cases.py:
every case's tensors go to the device, the real `ops.<op>` runs through Replay.run, and the launch must leave no failure, a ratio
<= 1, its inputs bit-identical and every byte outside its output slices untouched (the checker's check_outside).  Beyond the
checkers: ema_update equals the numpy float32 expression of model/EMA.py bit for bit, dropblock_mask its numpy restatement, the
off-centre taps of a 3x3 weight gradient on a 1x1 map are exactly 0, and every case gives identical bits on a second call from the
same state.  Replay.report() is printed per family of ops at the end of the module (profiles/train_edges_census.txt is the per-case
record of one run: a record, not a threshold)."""
import collections
import os

import pytest
import torch

import launch_replay as lr
import train_edge_cases as tec
from test_train_edge_cases import call_args, ema_reference, weight_cache_stub
from train_edge_cases import CASES

pytestmark = pytest.mark.gpu

CENSUS = collections.OrderedDict()
REPORTS = collections.OrderedDict()                   # family of ops -> census records of its launches


def family_of(op):
    if op.startswith('bn_'):
        return 'BatchNorm'
    if op.startswith('conv'):
        return 'contractions'
    if op in ('maxpool3x3s2', 'maxpool3x3s2_bwd', 'spp', 'spp_bwd', 'dropblock_mask'):
        return 'pooling'
    return 'element-wise ops, copies and small reductions'


def to_device(kw):
    """The case's CPU tensors on the device; tensors shared between arguments stay shared."""
    from ppyolo_hip import ops
    memo = {}

    def mv(v):
        if torch.is_tensor(v):
            if id(v) not in memo:
                memo[id(v)] = v.cuda()
            return memo[id(v)]
        if isinstance(v, ops.View):
            return ops.View(mv(v.t), v.coff, v.C)
        if isinstance(v, dict):
            return {k: mv(x) for k, x in v.items()}
        if isinstance(v, (tuple, list)):
            return type(v)(mv(x) for x in v)
        return v
    return collections.OrderedDict((k, mv(v)) for k, v in kw.items())


def _tensors(v, out):
    from ppyolo_hip import ops
    if torch.is_tensor(v):
        out.append(v)
    elif isinstance(v, ops.View):
        out.append(v.t)
    elif isinstance(v, dict):
        for x in v.values():
            _tensors(x, out)
    elif isinstance(v, (tuple, list)):
        for x in v:
            _tensors(x, out)
    return out


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.fixture(scope='module', autouse=True)
def census_report():
    yield
    from ppyolo_hip import ops
    print('\ntrain edge census: %d cases' % len(CENSUS))
    for fam, recs in REPORTS.items():                  # Replay.report() per family of ops
        rep = lr.Replay(ops)
        rep.census = recs
        print(rep.report('edge table, %s' % fam))
    out = os.environ.get('PPY_TRAIN_EDGES_CENSUS')
    if out:
        with open(out, 'w') as f:
            f.write('# op  case  worst err/bound of the launch (tests/test_gpu_train_edges.py on an MI355X; a record, the threshold is 1.0)\n')
            for name, (op, ratio) in CENSUS.items():
                f.write('%-22s %-52s %.4f\n' % (op, name, ratio))


@pytest.mark.parametrize('name', list(CASES))
def test_edge_case_through_the_launch_checker(name):
    from ppyolo_hip import ops
    case = CASES[name]
    fn = getattr(ops, case.op)
    old_env = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    try:
        kw = to_device(case.build())
        if case.prep is not None:
            case.prep(ops, kw)
        args = call_args(kw)
        bound = lr.Replay.bind(fn, **args)
        before = [(t, t.clone()) for t in _tensors(list(args.values()), [])]
        rep = lr.Replay(ops, weight_cache_stub(kw))
        rep.run(case.op, bound, lambda: fn(**args))
        torch.cuda.synchronize()
        assert not rep.failures, rep.report(name)
        rec = rep.census[-1]
        assert rec['checks'] and rec['ratio'] <= 1.0, rep.report(name)
        CENSUS[name] = (case.op, rec['ratio'])
        REPORTS.setdefault(family_of(case.op), []).append(rec)
        # inputs bit-identical afterwards
        outs = OUTPUTS[case.op]
        out_ptrs = {t.data_ptr() for k in outs if args.get(k) is not None for t in _tensors(args[k], [])}
        for t, b in before:
            if t.data_ptr() not in out_ptrs:
                assert torch.equal(_bits(t), _bits(b)), '%s: an input changed' % name
        extra_checks(case, kw, args)
        # a second call from the same state gives the same bits: every op of the table, reductions and split reductions included
        first = [t.clone() for k in outs if args.get(k) is not None for t in _tensors(args[k], [])]
        for t, b in before:                           # outputs (in-place ones too: running statistics, dst, dx) start from the same state
            if t.data_ptr() in out_ptrs:
                t.copy_(b)
        fn(**args)
        torch.cuda.synchronize()
        second = [t for k in outs if args.get(k) is not None for t in _tensors(args[k], [])]
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, second)), '%s: a second call gives other bits' % name
    finally:
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# arguments an op writes (everything else must come back bit-identical)
OUTPUTS = {
    'bn_train_stats': ('mean', 'invstd', 'running_mean', 'running_var', 'ws'), 'bn_train_stats_merge': ('mean', 'invstd', 'running_mean', 'running_var', 'partials'),
    'bn_train_apply': ('y', 'amax_out'), 'bn_train_bwd': ('dx', 'dgamma', 'dbeta', 'ws', 'amax_dx'), 'act_bwd': ('dx',), 'add_inplace': ('dst',),
    'dropblock_apply': ('y',), 'upsample2x': ('y',), 'upsample2x_bwd': ('dx',), 'avgpool2x2': ('y',), 'avgpool2x2_bwd': ('dx',), 'zero_insert': ('up',),
    'channel_sum': ('out', 'ws'), 'sgd_momentum': ('param', 'velocity'), 'ema_update': ('shadow',), 'maxpool3x3s2': ('y',), 'maxpool3x3s2_bwd': ('dx',),
    'spp': ('y5', 'y9', 'y13'), 'spp_bwd': ('dx', 'ws'), 'dropblock_mask': ('mask', 'scale', 'ws'), 'conv2d_wgrad': ('dw_krsc', 'ws'),
    'conv2d_dgrad': ('dx', 'ws'), 'conv2d_dgrad_prepared': ('dx', 'ws'), 'conv2d_train_fwd': ('y', 'partials'), 'conv1x1_stats': ('partials',),
    'conv1x1_bn_apply': ('y', 'amax_out'), 'conv2d_bn_act': ('y', 'amax_out', 'ws'),
}


def extra_checks(case, kw, args):
    """The exact assertions beyond the checker."""
    cpu = case.build() if case.op in ('ema_update', 'dropblock_mask') else None
    if case.op == 'ema_update':
        _, want = ema_reference(cpu['shadow'], cpu['param'], cpu['step'], cpu['ema_decay'])
        assert torch.equal(_bits(args['shadow'].cpu()), _bits(want)), '%s: not the three roundings of model/EMA.py' % case.name
    if case.op == 'dropblock_mask':
        N, H, W, C = cpu['mask'].shape
        want = tec.dropblock_mask_reference(N, H, W, C, cpu['keep_prob'], cpu['seed'])
        assert torch.equal(args['mask'].cpu().permute(0, 3, 1, 2), want), case.name
        if cpu['keep_prob'] == 1.0:
            assert float(args['scale']) == 1.0 and bool((args['mask'] == 1).all())
    if case.op == 'conv2d_wgrad' and '1x1map' in case.name:
        dw = args['dw_krsc'].clone()
        dw[:, 1, 1, :] = 0.0
        assert bool((dw == 0).all()), '%s: an off-centre tap of a 1 x 1 map is not exactly 0' % case.name
    if case.op == 'avgpool2x2_bwd':
        dx = tec.dense(args['dx'])
        H, W = dx.shape[1], dx.shape[2]
        assert bool((dx[:, H // 2 * 2:] == 0).all()) and bool((dx[:, :, W // 2 * 2:] == 0).all()), case.name


def test_every_op_of_the_table_names_its_outputs():
    assert {c.op for c in CASES.values()} <= set(OUTPUTS)
