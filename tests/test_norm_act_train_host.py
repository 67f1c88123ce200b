"""GroupNorm / AffineChannel / Mish in the training step, without a device: the torch restatement (tests/norm_act_train_ref.py)
against the reference's float32 and float64 rows of tests/golden/g24_norm_act_train*.npz (tools/make_goldens_g24.py), what
train_plan decides for such units, and the header's new symbols."""
import json
import os
import re

import pytest
import torch

import norm_act_ref as R
import norm_act_train_plan_dump as D
import norm_act_train_ref as T
from conftest import build_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from ppyolo_hip import train_plan as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = T.unit_cases()
GOLDEN_THREADS = 8          # the thread count the fixtures were made with (torch's reductions split by it)


def _cfg(cfgc, backbone, head):
    cfg = cfgc()
    cfg.backbone['norm_type'], cfg.head['norm_type'] = backbone, head
    return cfg


# ---- (a) the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', UNITS, ids=[T.case_id(c) for c in UNITS])
def test_restatement_equals_the_reference(case):
    """float32: the ATen calls the reference's modules make, so bit for bit at the fixture's thread count (as tests/test_oracle_golden.py
    pins it).  float64 (slopes locked to the golden's float32 signs, which are its float64 signs: asserted when the fixture was made):
    the stored rows are float32 differences, exact to 2^-24 of the difference; 1e-6 of it (and 1e-12) is asserted."""
    p, meta, x, dy, sd = case
    d = T.unit_files()
    threads = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)
    try:
        r32 = T.unit_fwd_bwd(meta, sd, x, dy)
    finally:
        torch.set_num_threads(threads)
    mask = (T.f32(d, p + 'y') > 0) if meta['act'] in ('relu', 'leaky') else None
    r64 = T.unit_fwd_bwd(meta, sd, x.double(), dy.double(), mask)
    rows = [('y', r32['y'], r64['y']), ('dx', r32['dx'], r64['dx'])] + [('g.' + k, v, r64['grads'][k]) for k, v in sorted(r32['grads'].items())]
    assert sorted(k for k, _, _ in rows) == sorted(k[len(p):] for k in d if k.startswith(p) and not k.endswith('.d64')
                                                   and k[len(p):].split('.')[0] in ('y', 'dx', 'g'))
    for key, a32, a64 in rows:
        assert torch.equal(a32, T.f32(d, p + key)), key
        own = torch.from_numpy(d[p + key + '.d64']).abs().max().item()
        assert (a64 - T.f64(d, p + key)).abs().max().item() <= 1e-6 * own + 1e-12, key


@pytest.mark.parametrize('case', UNITS, ids=[T.case_id(c) for c in UNITS])
def test_written_out_formulas_are_the_autograd_result(case):
    """gn_fwd_bwd / af_fwd_bwd / bn_fwd_bwd -- the formulas of include/ppyolo_hip.h, which the kernel tests measure against -- agree in
    float64 with autograd through the reference's own calls: 1e-9 of each tensor's maximum.  `one` (m = 1): the formula's dx is
    exactly 0, autograd's is rounding noise of rstd = 316: below 1e-9 absolute."""
    p, meta, x, dy, sd = case
    a = T.unit_fwd_bwd(meta, sd, x.double(), dy.double())
    b = T.unit_formulas(meta, sd, x.double(), dy.double())
    for key, u, v in [('y', a['y'], b['y']), ('dx', a['dx'], b['dx'])] + [(k, a['grads'][k], b['grads'][k]) for k in a['grads']]:
        assert (u - v).abs().max().item() <= 1e-9 * max(1.0, u.abs().max().item()), (p, key)
    if meta['special'] == 'one':
        assert float(b['dx'].abs().max()) == 0.0 and float(b['grads']['conv.weight'].abs().max()) == 0.0


def test_special_cases_are_what_they_claim():
    by = {c[1]['special']: c for c in UNITS if c[1]['special']}
    d = T.unit_files()
    p, meta, x, dy, sd = by['one']
    assert x.shape[2:] == (1, 1) and meta['cout'] == meta['groups']                       # m = 1
    p, meta, x, dy, sd = by['const']
    raw = torch.nn.functional.conv2d(x, sd['conv.weight'], sd['conv.bias'])[:, :2]
    assert float(raw.min()) == float(raw.max())                                            # group 0 is constant: rstd = 1 / sqrt(eps)
    p, meta, x, dy, sd = by['mean']
    raw = torch.nn.functional.conv2d(x.double(), sd['conv.weight'].double(), sd['conv.bias'].double())[:, 2:4]
    assert 990 < raw.mean().item() < 1010 and 1e-3 < raw.std().item() < 1e-1
    p, meta, x, dy, sd = by['mish']
    for v in T.MISH_PROBE:
        assert bool((x == torch.tensor(v)).any()), v
    # the derivative at the probe values, float64 formula against the golden's float64 row (dx / dy: identity convolution, af = 1, 0)
    g = T.f64(d, p + 'dx') / dy.double()
    assert (g - T.mish_grad(x.double())).abs().max().item() <= 1e-6
    assert bool((T.mish_grad(torch.tensor([20.01, 100.0])) == 1.0).all())
    for c in UNITS:          # relu / leaky: float32 and float64 agree on every sign (so a twin locked to either is the float64 row)
        if c[1]['act'] in ('relu', 'leaky'):
            assert bool(((T.f32(d, c[0] + 'y') > 0) == (T.f64(d, c[0] + 'y') > 0)).all()), c[0]


def test_mish_derivative_formula():
    x = torch.linspace(-30, 25, 2201, dtype=torch.float64).requires_grad_(True)
    R.mish(x).sum().backward()
    assert (T.mish_grad(x.detach()) - x.grad).abs().max().item() <= 1e-12


# ---- (b) train_plan -----------------------------------------------------------------------------------------------------------
def test_norm_form_of_every_unit_kind():
    want = {('bn', None): 'bn', ('bn', 'relu'): 'bn', ('bn', 'leaky'): 'bn', ('bn', 'mish'): 'bn_mish',
            ('gn', None): 'gn', ('gn', 'relu'): 'gn', ('gn', 'leaky'): 'gn', ('gn', 'mish'): 'gn',
            (None, None): 'none', (None, 'leaky'): 'none'}
    for (norm, act), form in want.items():
        for trainable in (False, True):
            assert TP.norm_form(norm, act, trainable) == form, (norm, act, trainable)
    for act, frozen in ((None, 'af_fold'), ('relu', 'af_fold'), ('leaky', 'af_fold'), ('mish', 'af_fold_mish')):
        assert TP.norm_form('af', act, False) == frozen and TP.norm_form('af', act, True) == 'af_train'
    with pytest.raises(ValueError):
        TP.norm_form(None, 'mish', True)
    with pytest.raises(ValueError):
        TP.norm_form('gn', 'swish', True)
    keys = {'a.conv.weight', 'a.gn.weight', 'a.gn.bias', 'b.conv.weight', 'b.af.weight', 'c.conv.weight', 'c.bn.weight', 'd.conv.weight'}
    assert [TP.norm_of(keys, p) for p in 'abcd'] == ['gn', 'af', 'bn', None]


def test_refusals_name_the_unit():
    assert TP.norm_refusal('u', 'bn', 4096, 1, 0.5) is None                         # BatchNorm units: as before
    assert TP.norm_refusal('head.x (n)', 'gn', 256, 32, 0.0) is None and TP.norm_refusal('u', 'af', 4096, 1, 0.0) is None
    assert 'head.x (n)' in TP.norm_refusal('head.x (n)', 'gn', 48, 32, 0.0) and 'C % groups' in TP.norm_refusal('u', 'gn', 48, 32, 0.0)
    assert '2048' in TP.norm_refusal('u', 'gn', 4096, 32, 0.0)
    assert 'norm_decay' in TP.norm_refusal('u', 'gn', 64, 32, 5e-4) and 'norm_decay' in TP.norm_refusal('u', 'af', 64, 1, 5e-4)


@pytest.mark.parametrize('cfgc,bb,hd,fa', [(PPYOLO_r18vd_Config, 'bn', 'gn', 5), (PPYOLO_r18vd_Config, 'gn', 'gn', 4),
                                            (PPYOLO_2x_Config, 'affine_channel', 'gn', 5), (PPYOLO_2x_Config, 'affine_channel', 'affine_channel', 3)])
def test_flat_layout_puts_the_norm_parameters_behind_n_decay(cfgc, bb, hd, fa):
    model, _ = build_model(_cfg(cfgc, bb, hd))
    params = [(k, TP.kernel_shape(tuple(q.shape))) for k, q in model.named_parameters() if TP.stage_of(k) > fa]
    layout, total, n_decay = TP.flat_layout(params)
    tails = ('.gn.weight', '.gn.bias', '.af.weight', '.af.bias')
    news = [k for k, _ in params if k.endswith(tails)]
    assert news and all(layout[k][0] >= n_decay for k in news)
    assert all((layout[k][0] < n_decay) == (len(s) == 4 or k.endswith('.conv_offset.bias')) for k, s in params)
    for k in news:
        assert TP.unit_of(k) == k.rsplit('.', 2)[0] and TP.unit_of(k) + '.conv.weight' in layout or TP.unit_of(k) + '.conv.dcn_weight' in layout
    bk = TP.buckets([k for k, _ in params], layout, total)
    for k in news:
        assert TP.unit_of(k) in bk[TP.bucket_of(k)]['units']


def test_batch_norm_decisions_are_the_parent_commit_s():
    """conv_form over a grid of its arguments and the flat layout / units / buckets of both shipped configurations, against the
    digests tests/norm_act_train_plan_dump.py took with the parent commit's train_plan.py (the dump itself is 300 KB)."""
    want = json.load(open(os.path.join(R.GOLDEN, 'g24_train_plan_parent.json')))
    got = D.digests(D.dump(TP, D.shipped_param_shapes()))
    assert got == want
    assert want['conv_form']['rows'] > 3000 and len(want) == 7
    for name, params in D.shipped_param_shapes().items():          # ... and every unit of a shipped model is 'bn' / 'none'
        keys = {k for k, _ in params}
        assert {TP.norm_form(TP.norm_of(keys, TP.unit_of(k)), 'leaky', t) for k in keys for t in (False, True)} == {'bn', 'none'}


def test_train_step_builds_its_refusals_from_the_model():
    from ppyolo_hip.train_norm import norm_units
    from ppyolo_hip._lib import PPYoloHipError
    model, _ = build_model(_cfg(PPYOLO_r18vd_Config, 'bn', 'gn'))
    gn = norm_units(model)
    assert gn and all(v == (32, 1e-5) for v in gn.values()) and all(k.startswith('head.') for k in gn)
    assert norm_units(build_model(PPYOLO_r18vd_Config())[0]) == {}
    unit = model.head.detection_blocks[0].layers[2]
    unit.norm_decay = 5e-4
    with pytest.raises(PPYoloHipError, match=r'head\.detection_blocks\.0\.layers\.2 \(\S+\): norm_decay'):
        norm_units(model)
    unit.norm_decay = 0.0
    unit.gn.num_groups = 24
    with pytest.raises(PPYoloHipError, match=r'head\.detection_blocks\.0\.layers\.2 .*C % groups'):
        norm_units(model)


# ---- (c) the header -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_training_entry_points():
    text = open(os.path.join(ROOT, 'include', 'ppyolo_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    from ppyolo_hip import _lib
    for name in ('ppy_group_norm_train_f32', 'ppy_group_norm_bwd_workspace_bytes', 'ppy_group_norm_bwd_f32', 'ppy_affine_act_f32',
                 'ppy_affine_bwd_workspace_bytes', 'ppy_affine_bwd_f32', 'ppy_mish_bwd_f32'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.exported_symbols(), name
        assert name in text.replace(code, '') or name in text          # (documented in the contract comment)
