"""What train_plan decides for BatchNorm models, dumped: conv_form over a grid of its arguments and the flat layout / unit prefixes /
buckets of the two shipped configurations at three freeze_at values.  tests/golden/g24_train_plan_parent.json holds the digests (rows, sha256 per section) of this dump taken with
the train_plan.py of the commit before GroupNorm / AffineChannel / Mish reached the training step:

    python tests/norm_act_train_plan_dump.py path/to/that/train_plan.py > tests/golden/g24_train_plan_parent.json
"""
import collections
import hashlib
import importlib.util
import itertools
import json
import os
import sys

Cfg = collections.namedtuple('Cfg', 'id family local splitk_mode bn_stats stats_twin')
TILES = [Cfg(0, 'f16x2', 0, 'workspace', True, -1), Cfg(1, 'bf16x3', 0, 'workspace', False, -1), Cfg(2, 'stream', 0, 'none', True, -1),
         Cfg(3, 'stream', 1, 'none', True, -1), Cfg(4, 'kparity', 0, 'workspace', False, 0), Cfg(5, 'small', 0, 'workgroup', False, -1)]
STREAM0 = 2


def dump(TP, param_shapes):
    """param_shapes: {config name: [(parameter key, shape)]} of the shipped (BatchNorm) models."""
    out = {'conv_form': [], 'layout': {}}
    envs = [{}, {'PPYOLO_HIP_TRAIN_BN_EPILOGUE': '1'}, {'PPYOLO_HIP_TRAIN_MATH': 'fp32'}]
    for env in envs:
        sw = TP.switches(env, 1, False, False)
        for has_bn, f16, trainable, coord in itertools.product((True, False), repeat=4):
            for (R, stride), (C, Kout, HW), table in itertools.product(((1, 1), (3, 1), (3, 2)), ((128, 512, 5776), (128, 384, 16), (256, 512, 361)),
                                                                       ((0, 1), (0, 2), (1, 1), (3, 1), (4, 2), (5, 2), (-1, 0))):
                got = TP.conv_form(has_bn, f16, trainable, coord, R, R, stride, C, Kout, HW, table, sw, TILES.__getitem__, STREAM0)
                out['conv_form'].append([sorted(env), has_bn, f16, trainable, coord, R, stride, C, Kout, HW, list(table), list(got)])
    for name, params in sorted(param_shapes.items()):
        for fa in (5, 3, 0):
            keyed = [(k, TP.kernel_shape(tuple(s))) for k, s in params if TP.stage_of(k) > fa]
            layout, total, n_decay = TP.flat_layout(keyed)
            bk = TP.buckets([k for k, _ in keyed], layout, total)
            out['layout']['%s:%d' % (name, fa)] = dict(
                total=total, n_decay=n_decay, offsets=[[k, layout[k][0], layout[k][1]] for k, _ in keyed],
                units=sorted({TP.unit_of(k) for k, _ in keyed}),
                buckets={b: dict(units=sorted(v['units']), ranges=[list(r) for r in v['ranges']]) for b, v in sorted(bk.items())})
    return out


def digests(d):
    """{section: {rows, sha256}} of a dump: what the fixture keeps."""
    def one(v):
        rows = len(v) if isinstance(v, list) else len(v['offsets'])
        return dict(rows=rows, sha256=hashlib.sha256(json.dumps(v, sort_keys=True, separators=(',', ':')).encode()).hexdigest())
    out = {'conv_form': one(d['conv_form'])}
    out.update({'layout ' + k: one(v) for k, v in d['layout'].items()})
    return out


def shipped_param_shapes():
    from conftest import build_model
    from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
    return {name: [(k, tuple(p.shape)) for k, p in build_model(cfgc(), 0, 'cpu')[0].named_parameters()]
            for name, cfgc in (('r50vd', PPYOLO_2x_Config), ('r18vd', PPYOLO_r18vd_Config))}


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(here, '..', 'pytorch-ppyolo_amd'), os.path.join(here, '..')]
    spec = importlib.util.spec_from_file_location('train_plan_other', sys.argv[1])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    json.dump(digests(dump(mod, shipped_param_shapes())), sys.stdout, sort_keys=True, indent=1)
