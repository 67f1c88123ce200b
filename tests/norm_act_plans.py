"""Device-free derivation of a model's skeleton plan with its link state, and a dump of it (tests/test_norm_act_host.py).

derive(): the order HipExecutor follows (plan_links.py) -- assign_amax, link_pools, link_maxpools, the 'gp_in' candidates, the
committed measured table, decide_links -- over a skeleton plan (shapes only), as tests/test_plan_host_logic.py does for the bench plan.
dump(): one line per op holding op kinds, shapes, link flags and tile ids only.

    python tests/norm_act_plans.py OUT.json      # writes the dump of the two shipped configurations at S = 608, 416, 320
"""
import json
import os
import sys

SIZES = (608, 416, 320)
BATCH = 8


def derive(model, N, S):
    from ppyolo_hip import ops as K
    from ppyolo_hip import plan_links as L
    from ppyolo_hip.engine import _TUNED_PATHS
    from ppyolo_hip.runtime import build_plan
    plan = build_plan(model, N, S, S, 'cpu', skeleton=True)
    for op in plan.ops:
        if op['op'] in ('conv', 'dcn'):
            op['wf16'] = True           # (the executor's split fp16 weights: the rules only ask whether they are there)
    pinned = {a.buf for a in list(plan.head_outs) + list(plan.feats)}
    L.assign_amax(plan.ops)
    L.link_pools(L.BufferIndex(plan.ops), L.has_f16)
    L.link_maxpools(L.BufferIndex(plan.ops), pinned, L.has_f16)
    index = L.BufferIndex(plan.ops)
    for _, cons in L.split_pairs(index, plan.buffers, pinned, L.has_f16):
        for c in cons:
            c['gp_in'] = True
    tabs = [json.load(open(_TUNED_PATHS[m])) for m in ('f16x2', 'bf16x3')]
    L.apply_tuned(plan.ops, *tabs)
    links, fused, _ = L.decide_links(plan.ops, index, plan.buffers, pinned, L.has_f16, K.conv_cfg)
    return plan, links, fused


def _a(a):
    return None if a is None else [a.buf, a.coff, a.C, a.N, a.H, a.W]


def dump(plan, links, fused):
    pos = {id(op): i for i, op in enumerate(plan.ops)}
    prod = {pr: cons for pr, cons in links}
    cons_of = {c: pr for pr, cons in links for c in cons}
    first, second = {a: b for a, b in fused}, {b: a for a, b in fused}
    out = []
    for i, op in enumerate(plan.ops):
        rec = dict(op=op['op'], stream=op.get('stream', 0))
        for k in ('x', 'y', 'res', 'posb', 'om', 'y5', 'y9', 'y13', 'pool', 'mpool'):
            if op.get(k) is not None:
                rec[k] = _a(op[k])
        if op.get('w') is not None:
            rec['w'] = list(op['w'].shape)
        for k in ('stride', 'pad', 'act', 'ups', 'cfg', 'splitk', 'amax_in_id', 'amax_in2_id', 'amax_out_id', 'gp_in'):
            if op.get(k) is not None:
                rec[k] = op[k]
        if op.get('owner') is not None:
            rec['owner'] = pos[id(op['owner'])]
        if i in prod:
            rec['presplit_to'] = prod[i]
        if i in cons_of:
            rec['presplit_from'] = cons_of[i]
        if i in first:
            rec['b2b'] = first[i]
        if i in second:
            rec['b2b_of'] = second[i]
        out.append(json.dumps(rec, sort_keys=True))
    return dict(buffers=[list(b) for b in plan.buffers], ops=out)


def shipped_dumps():
    from conftest import build_model
    from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
    res = {}
    for tag, cfgc in (('r50vd', PPYOLO_2x_Config), ('r18vd', PPYOLO_r18vd_Config)):
        model, _ = build_model(cfgc())
        for S in SIZES:
            res['%s_%d' % (tag, S)] = dump(*derive(model, BATCH, S))
    return res


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest  # noqa: F401  (puts the package on the path)
    with open(sys.argv[1], 'w') as fh:
        json.dump(shipped_dumps(), fh, indent=0, sort_keys=True)
