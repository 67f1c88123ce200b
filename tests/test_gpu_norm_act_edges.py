"""The GroupNorm / AffineChannel / Mish kernels on the edge table of tests/norm_act_edge_cases.py, on the MI355X.

One runner per `op` of the table (RUNNERS).  A runner talks to the kernels through a small adaptor (Device below) so that
tests/test_norm_act_edge_cases.py can hand the SAME runner a CPU stand-in: what is asserted here is then known to be fair (a plain
float32 implementation passes) and sharp (a planted fault fails) before a kernel ever runs.

Bounds -- all of them are those of the direct tests, none is new:
  forward against float64 on the same float32 input: 16 * ULP * max(1, S), as test_group_norm_kernel (tests/test_gpu_norm_act.py)
    derives it;
  backward (and the AffineChannel forward): norm_act_train_ref.judge with K_GN = 3 and its floor 1e-6, as
    tests/test_gpu_norm_act_train.py -- max |hip - f64| <= 3 * max |f32 restatement - f64| + 1e-6 * max |f64| on the device's own
    slope mask.  Where a case carries a `twin` (a group with a mean near 1000: the float32 restatement loses that group's variance and
    is no yardstick), the restatement's error is taken on the twin -- the same data with that group shifted by an exactly
    representable amount, GroupNorm being shift-invariant per group -- and the float64 reference on the original input; same
    factor, same floor;
  Mish: 16 * ULP relative (+ 1e-37) as test_mish_kernel; its derivative: the 4-ulp rule of test_mish_backward_kernel, and with a scale
    and a shift that test's bound.
Everything else is an exact statement.  Every test prints one `NORM-ACT-EDGES <case> ...` line: the worst item's error, its yardstick,
its bound and error / bound (profiles/norm_act_edges_census.txt holds a run's lines)."""
import numpy as np
import pytest
import torch

import norm_act_edge_cases as E
import norm_act_ref as R
import norm_act_train_ref as T
from norm_act_edge_cases import CASES, SENTINEL, chosen_of, dense
from ppyolo_hip import ops as K

pytestmark = pytest.mark.gpu

K_GN = 3.0          # tests/test_gpu_norm_act_train.py
ULP = 2.0 ** -24    # tests/test_gpu_norm_act.py
LEAKY = torch.tensor(0.1, dtype=torch.float32)


class Device(object):
    """The kernels behind the interface the runners use.  train=False is the raw call with param_grads = 0 and the caller's
    gradient pointers still handed over: they must come back untouched."""
    exact = True          # exact statements are asserted (a plain float32 restatement on the CPU is held to the bounds only)

    def put(self, t):
        return None if t is None else t.cuda()

    def view(self, v):
        return None if v is None else K.View(v.t.cuda(), v.coff, v.C)

    def host(self, v):
        torch.cuda.synchronize()
        return K.View(v.t.cpu(), v.coff, v.C)

    def get(self, t):
        torch.cuda.synchronize()
        return t.cpu()

    def stats(self, n):
        return torch.zeros(n, dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.float32, device='cuda')

    def group_norm(self, x, g, b, groups, eps, y, act, res, upsample2x=False):
        K.group_norm(x, g, b, groups, eps, y, act, res, upsample2x=upsample2x)

    def group_norm_train(self, x, g, b, groups, eps, y, mean, rstd, act, res):
        K.group_norm_train(x, g, b, groups, eps, y, mean, rstd, act, res)

    def group_norm_bwd(self, x, mean, rstd, g, b, groups, dy, dx, act, res, dz, dgamma, dbeta, train=True):
        if train:
            K.group_norm_bwd(x, mean, rstd, g, b, groups, dy, dx, act, res, dz, dgamma, dbeta)
            return
        from ppyolo_hip._lib import NORM_ACT, check, lib
        ws = torch.empty(int(lib().ppy_group_norm_bwd_workspace_bytes(x.N, x.H, x.W, x.C, groups)) // 4 + 2, device='cuda')
        check(lib().ppy_group_norm_bwd_f32(x.ptr, x.ld, mean.data_ptr(), rstd.data_ptr(), g.data_ptr(), b.data_ptr(), groups, NORM_ACT[act],
                                           None if res is None else res.ptr, 0 if res is None else res.ld, dy.ptr, dy.ld, dx.ptr, dx.ld,
                                           None if dz is None else dz.ptr, 0 if dz is None else dz.ld, dgamma.data_ptr(), dbeta.data_ptr(), 0,
                                           x.N, x.H, x.W, x.C, ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream),
              'ppy_group_norm_bwd_f32')

    def affine_act(self, x, w, b, y, act, res):
        K.affine_act(x, w, b, y, act, res)

    def affine_bwd(self, x, w, b, dy, dx, act, res, dz, dw, db, train=True):
        if train:
            K.affine_bwd(x, w, b, dy, dx, act, res, dz, dw, db)
            return
        from ppyolo_hip._lib import NORM_ACT, check, lib
        check(lib().ppy_affine_bwd_f32(x.ptr, x.ld, w.data_ptr(), b.data_ptr(), NORM_ACT[act], None if res is None else res.ptr,
                                       0 if res is None else res.ld, dy.ptr, dy.ld, dx.ptr, dx.ld, None if dz is None else dz.ptr,
                                       0 if dz is None else dz.ld, dw.data_ptr(), db.data_ptr(), 0, x.N, x.H, x.W, x.C, None, 0,
                                       torch.cuda.current_stream().cuda_stream), 'ppy_affine_bwd_f32')

    def mish(self, v):
        K.mish(v)

    def mish_bwd(self, x, dy, dx, scale, shift):
        K.mish_bwd(x, dy, dx, scale, shift)


class Report(object):
    """What a runner measured: items (what, error, yardstick, bound) and free-form notes, printed as one line."""

    def __init__(self, case):
        self.case, self.items, self.notes = case, [], []

    def add(self, what, err, yard, bound):
        self.items.append((what, err, yard, bound))

    def worst(self):
        return max(self.items, key=lambda it: it[1] / max(it[3], 1e-300)) if self.items else None

    def line(self):
        w = self.worst()
        s = 'NORM-ACT-EDGES %-46s %-14s' % (self.case.name, self.case.op)
        if w:
            s += ' worst %-8s err %.3e  yardstick %.3e  bound %.3e  ratio %.3f' % (w[0], w[1], w[2], w[3], w[1] / max(w[3], 1e-300))
        return s + ''.join('  [%s]' % n for n in self.notes)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _act32(u, act):
    """relu / leaky of a float32 tensor with the kernel's own expression (v > 0 ? v : v * 0.1f)."""
    return torch.where(u > 0, u, u * (LEAKY if act == 'leaky' else 0.0)) if act in ('relu', 'leaky') else u


def _untouched(D, dev_views, cpu_views, names):
    for k in names:
        if dev_views[k] is not None:
            assert torch.equal(D.host(dev_views[k]).t, cpu_views[k].t), 'input %s was written' % k


def _refill(v):
    v.t.fill_(SENTINEL)


def _forward_bound(rep, what, got_nhwc, kw, x=None):
    """float64 two-pass GroupNorm on the same float32 input; S = max |xhat gamma + beta| + max |res|."""
    x = kw['x'] if x is None else x
    y = R.group_norm_two_pass(_nchw(x.double()), kw['gamma'].double(), kw['beta'].double(), kw['groups'], kw['eps'])
    S = y.abs().max().item() + (kw['res'].abs().max().item() if kw['res'] is not None else 0.0)
    pre = y + (_nchw(kw['res'].double()) if kw['res'] is not None else 0.0)
    ref = R.act(pre, kw['act']).permute(0, 2, 3, 1)
    err = (got_nhwc.double() - ref).abs().max().item()
    bound = 16 * ULP * max(1.0, S)
    rep.add(what, err, bound, bound)
    assert err <= bound, '%s %s: %.3e against float64, bound %.3e' % (rep.case.name, what, err, bound)


def _judge(rep, what, got, r32, r64y, r64):
    """norm_act_train_ref.judge; r64y is the float64 row the float32 restatement is measured against (the twin's, or r64 itself)."""
    e_got = (got.double() - r64.double()).abs().max().item()
    e_ref = (r32.double() - r64y.double()).abs().max().item()
    bound = K_GN * e_ref + 1e-6 * r64.double().abs().max().item()
    rep.add(what, e_got, e_ref, bound)
    if r64y is r64:
        T.judge('%s %s' % (rep.case.name, what), got, r32, r64, K_GN)
    assert e_got <= bound, '%s %s: %.3e against float64, bound %.3e (the float32 restatement: %.3e)' % (rep.case.name, what, e_got, bound, e_ref)


# ---- GroupNorm forward -------------------------------------------------------------------------------------------------------
def run_gn_fwd(case, kw, D, rep):
    N, H, W, C = kw['shape']
    G, act, eps = kw['groups'], kw['act'], kw['eps']
    V = E.gn_views(kw)
    dv = {k: D.view(V[k]) for k in ('x', 'res', 'y', 'yu')}
    g, b = D.put(kw['gamma']), D.put(kw['beta'])
    D.group_norm(dv['x'], g, b, G, eps, dv['y'], act, dv['res'])
    yh = D.host(dv['y'])
    first = dense(yh).clone()
    _forward_bound(rep, 'y', first, kw)
    assert E.outside_untouched(yh), 'written outside the slice'
    _refill(dv['y'])
    D.group_norm(dv['x'], g, b, G, eps, dv['y'], act, dv['res'])
    assert torch.equal(dense(D.host(dv['y'])), first), 'two runs differ'
    # the training forward: the same values, bit for bit, and the statistics
    _refill(dv['y'])
    mean, rstd = D.stats(N * G)
    D.group_norm_train(dv['x'], g, b, G, eps, dv['y'], mean, rstd, act, dv['res'])
    yh = D.host(dv['y'])
    assert torch.equal(dense(yh), first) and E.outside_untouched(yh), 'ppy_group_norm_train_f32 differs from ppy_group_norm_f32'
    # the 2 x 2 nearest-upsampled store: the plain result, repeated
    D.group_norm(dv['x'], g, b, G, eps, dv['yu'], act, dv['res'], upsample2x=True)
    yu = D.host(dv['yu'])
    assert torch.equal(dense(yu), first.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)) and E.outside_untouched(yu)
    _untouched(D, dv, V, ('x', 'res'))


# ---- GroupNorm training forward + backward -----------------------------------------------------------------------------------
def _gn_bwd_once(D, dv, st, g, b, G, act, C, train=True, fill=-5.5):
    dg, db = D.put(torch.full((C,), fill)), D.put(torch.full((C,), fill + 1.0))
    _refill(dv['dx'])
    _refill(dv['dz'])
    D.group_norm_bwd(dv['x'], st[0], st[1], g, b, G, dv['dy'], dv['dx'], act, dv['res'], dv['dz'], dg, db, train=train)
    dxh, dzh = D.host(dv['dx']), D.host(dv['dz'])
    assert E.outside_untouched(dxh) and E.outside_untouched(dzh), 'written outside the slice'
    return dense(dxh).clone(), dense(dzh).clone(), D.get(dg), D.get(db)


def _slope_check(rep, kw, D, y, dz, z):
    """(y > 0) == (dz == dy) over the whole tensor and on the chosen elements; elsewhere dz is 0 (relu) or 0.1f * dy (leaky)."""
    act, dy, ch = kw['act'], kw['dy'], kw['chosen']
    pos, one = y > 0, dz == dy
    other = torch.zeros_like(dy) if act == 'relu' else dy * LEAKY
    bad = (pos != one) | (~pos & (dz != other))
    zc = chosen_of(z, ch)
    rep.slope = dict(chosen=int(ch.shape[0]), pos=int((zc > 0).sum()), neg=int((zc < 0).sum()), zero=int((zc == 0).sum()),
                     disagree_chosen=int(chosen_of(bad, ch).sum()), disagree_all=int(bad.sum()))
    rep.notes.append('chosen z > 0: %(pos)d, z < 0: %(neg)d, z == 0: %(zero)d; disagreements: %(disagree_chosen)d chosen, %(disagree_all)d in all' % rep.slope)
    assert bool((chosen_of(pos, ch) == (zc > 0)).all()), 'the forward with and without the activation disagree on the sign of z'
    assert rep.slope['disagree_all'] == 0 and rep.slope['disagree_chosen'] == 0, rep.notes[-1]


def run_gn_train_bwd(case, kw, D, rep):
    N, H, W, C = kw['shape']
    G, act, eps, value = kw['groups'], kw['act'], kw['eps'], kw['value']
    V = E.gn_views(kw)
    dv = {k: D.view(V[k]) for k in ('x', 'dy', 'res', 'y', 'dx', 'dz')}
    g = D.put(kw['gamma'])
    if value == 'slope':
        # t = fl(xhat * gamma) as the device computes it (beta = 0, no activation, no residual), then beta_c = -t at channel c's element
        D.group_norm(dv['x'], g, D.put(torch.zeros(C)), G, eps, dv['y'], None, None)
        kw = dict(kw, beta=-chosen_of(dense(D.host(dv['y'])), kw['chosen']))
        _refill(dv['y'])
    b = D.put(kw['beta'])
    st = D.stats(N * G)
    D.group_norm_train(dv['x'], g, b, G, eps, dv['y'], st[0], st[1], act, dv['res'])
    yh = D.host(dv['y'])
    y = dense(yh).clone()
    assert E.outside_untouched(yh)
    _forward_bound(rep, 'y', y, kw)
    dx, dz, dg, db = _gn_bwd_once(D, dv, st, g, b, G, act, C)
    if value == 'slope':
        _refill(dv['y'])          # z itself: the forward once more, without the activation
        D.group_norm(dv['x'], g, b, G, eps, dv['y'], None, dv['res'])
        _slope_check(rep, kw, D, y, dz, dense(D.host(dv['y'])))
    # against float64 on the device's own slope mask
    mask = _nchw(y > 0) if act in ('relu', 'leaky') else None
    res = None if kw['res'] is None else _nchw(kw['res'])

    def ref(x, dt):
        return T.gn_fwd_bwd(_nchw(x).to(dt), kw['gamma'].to(dt), kw['beta'].to(dt), G, act, _nchw(kw['dy']).to(dt),
                            None if res is None else res.to(dt), mask, eps)
    r64 = ref(kw['x'], torch.float64)
    twin = kw.get('twin')
    r64y = r64 if twin is None else ref(twin, torch.float64)
    r32 = ref(kw['x'] if twin is None else twin, torch.float32)
    _judge(rep, 'dx', _nchw(dx), r32['dx'], r64y['dx'], r64['dx'])
    _judge(rep, 'dgamma', dg, r32['dgamma'], r64y['dgamma'], r64['dgamma'])
    _judge(rep, 'dbeta', db, r32['dbeta'], r64y['dbeta'], r64['dbeta'])
    _judge(rep, 'dz', _nchw(dz), r32['dz'], r64y['dz'], r64['dz'])
    if not D.exact:
        return
    # two runs are bit-identical; the frozen run gives the same dx / dz and leaves the gradient buffers alone
    dx2, dz2, dg2, db2 = _gn_bwd_once(D, dv, st, g, b, G, act, C)
    assert torch.equal(dx2, dx) and torch.equal(dz2, dz) and torch.equal(dg2, dg) and torch.equal(db2, db), 'two runs differ'
    dx3, dz3, keep_g, keep_b = _gn_bwd_once(D, dv, st, g, b, G, act, C, train=False, fill=3.5)
    assert torch.equal(dx3, dx) and torch.equal(dz3, dz), 'the frozen run gives another dx'
    assert bool((keep_g == 3.5).all()) and bool((keep_b == 4.5).all()), 'the frozen run wrote dgamma / dbeta'
    # the training forward is the inference forward
    _refill(dv['y'])
    D.group_norm(dv['x'], g, b, G, eps, dv['y'], act, dv['res'])
    assert torch.equal(dense(D.host(dv['y'])), y), 'ppy_group_norm_f32 differs from ppy_group_norm_train_f32'
    _untouched(D, dv, V, ('x', 'dy', 'res'))
    if value in ('constant_group', 'zero_preactivation'):
        n, gi = kw['sel']
        s = E._group_slice(C, G, gi)
        mean, rstd = D.get(st[0]), D.get(st[1])
        assert mean[n * G + gi].item() == kw['const'], 'the mean of a constant group is the constant'
        want = np.float32(1.0 / np.sqrt(np.float64(np.float32(eps))))
        assert rstd[n * G + gi].item() == float(want), 'var == 0: rstd %r, 1 / sqrt(eps) %r' % (rstd[n * G + gi].item(), float(want))
        u = kw['beta'][s].expand(H, W, -1)
        if kw['res'] is not None:
            u = u + kw['res'][n, :, :, s]
        assert torch.equal(y[n, :, :, s], _act32(u, act)), 'y on a constant group is act(beta [+ res]), bit for bit'
        dy1 = kw['dy'].clone()          # the group's share of dgamma from its image alone: xhat is exactly 0
        dy1[torch.arange(N) != n] = 0.0
        dv1 = dict(dv, dy=D.view(E.view(dy1, 12, 4)))
        _, _, dg1, _ = _gn_bwd_once(D, dv1, st, g, b, G, act, C)
        assert bool((dg1[s] == 0).all()), 'dgamma of a constant group: %r' % dg1[s].tolist()
        if value == 'zero_preactivation':
            assert bool((y[n, :, :, s] == 0).all()), 'z == 0: y == 0'
            want_dz = torch.zeros_like(kw['dy'][n, :, :, s]) if act == 'relu' else kw['dy'][n, :, :, s] * LEAKY
            assert torch.equal(dz[n, :, :, s], want_dz), 'z == 0 takes the slope of the negative side'
    if value == 'image_independence':
        for n in range(N):
            one = dict(kw, shape=(1, H, W, C), x=kw['x'][n:n + 1], dy=kw['dy'][n:n + 1], res=kw['res'][n:n + 1])
            v1 = {k: D.view(v) for k, v in E.gn_views(one).items() if k != 'yu'}
            s1 = D.stats(G)
            D.group_norm_train(v1['x'], g, b, G, eps, v1['y'], s1[0], s1[1], act, v1['res'])
            dxa, dza, _, _ = _gn_bwd_once(D, v1, s1, g, b, G, act, C)
            assert torch.equal(dense(D.host(v1['y']))[0], y[n]), 'y of image %d depends on the batch' % n
            assert torch.equal(dxa[0], dx[n]) and torch.equal(dza[0], dz[n]), 'dx / dz of image %d depend on the batch' % n


# ---- AffineChannel -----------------------------------------------------------------------------------------------------------
def _af_bwd_once(D, dv, w, b, act, C, train=True, fill=-5.5):
    dw, db = D.put(torch.full((C,), fill)), D.put(torch.full((C,), fill + 1.0))
    _refill(dv['dx'])
    _refill(dv['dz'])
    D.affine_bwd(dv['x'], w, b, dv['dy'], dv['dx'], act, dv['res'], dv['dz'], dw, db, train=train)
    dxh, dzh = D.host(dv['dx']), D.host(dv['dz'])
    assert E.outside_untouched(dxh) and E.outside_untouched(dzh), 'written outside the slice'
    return dense(dxh).clone(), dense(dzh).clone(), D.get(dw), D.get(db)


def run_affine_act_bwd(case, kw, D, rep):
    N, H, W, C = kw['shape']
    act = kw['act']
    V = E.af_views(kw)
    dv = {k: D.view(V[k]) for k in ('x', 'dy', 'res', 'y', 'dx', 'dz')}
    w, b = D.put(kw['gamma']), D.put(kw['beta'])
    D.affine_act(dv['x'], w, b, dv['y'], act, dv['res'])
    yh = D.host(dv['y'])
    y = dense(yh).clone()
    assert E.outside_untouched(yh)
    mask = _nchw(y > 0) if act in ('relu', 'leaky') else None
    res = None if kw['res'] is None else _nchw(kw['res'])

    def ref(dt):
        return T.af_fwd_bwd(_nchw(kw['x']).to(dt), kw['gamma'].to(dt), kw['beta'].to(dt), act, _nchw(kw['dy']).to(dt),
                            None if res is None else res.to(dt), mask)
    r32, r64 = ref(torch.float32), ref(torch.float64)
    dx, dz, dw, db = _af_bwd_once(D, dv, w, b, act, C)
    if kw['value'] == 'slope':
        _refill(dv['y'])
        D.affine_act(dv['x'], w, b, dv['y'], None, dv['res'])
        _slope_check(rep, kw, D, y, dz, dense(D.host(dv['y'])))
    _judge(rep, 'y', _nchw(y), r32['y'], r64['y'], r64['y'])
    _judge(rep, 'dx', _nchw(dx), r32['dx'], r64['dx'], r64['dx'])
    _judge(rep, 'dweight', dw, r32['dgamma'], r64['dgamma'], r64['dgamma'])
    _judge(rep, 'dbias', db, r32['dbeta'], r64['dbeta'], r64['dbeta'])
    _judge(rep, 'dz', _nchw(dz), r32['dz'], r64['dz'], r64['dz'])
    if not D.exact:
        return
    dx2, dz2, dw2, db2 = _af_bwd_once(D, dv, w, b, act, C)
    assert torch.equal(dx2, dx) and torch.equal(dz2, dz) and torch.equal(dw2, dw) and torch.equal(db2, db), 'two runs differ'
    dx3, dz3, keep_w, keep_b = _af_bwd_once(D, dv, w, b, act, C, train=False, fill=3.5)          # frozen, no workspace
    assert torch.equal(dx3, dx) and torch.equal(dz3, dz), 'the frozen run gives another dx'
    assert bool((keep_w == 3.5).all()) and bool((keep_b == 4.5).all()), 'the frozen run wrote dweight / dbias'
    _untouched(D, dv, V, ('x', 'dy', 'res'))


# ---- Mish ----------------------------------------------------------------------------------------------------------------------
def _ulp_of(r):          # tests/test_gpu_norm_act_train.py: of the reference, or of the smallest normal float32 below it
    return torch.maximum(r.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2().double() * 2.0 ** -23


def run_mish(case, kw, D, rep):
    V = E.mish_views(kw)
    v = D.view(V['x'])
    ref = R.mish(kw['x'].double())
    D.mish(v)
    h = D.host(v)
    got = dense(h).double()
    bound = 16 * ULP * ref.abs() + 1e-37
    err = (got - ref).abs()
    i = int((err / bound).argmax())
    rep.add('y', err.reshape(-1)[i].item(), bound.reshape(-1)[i].item(), bound.reshape(-1)[i].item())
    assert bool((err <= bound).all()), 'mish: %.3f of the bound at x = %r' % ((err / bound).max().item(), kw['x'].reshape(-1)[i].item())
    assert E.outside_untouched(h), 'in place, on the slice only'
    big = kw['x'] > 20
    assert torch.equal(dense(h)[big], kw['x'][big]), 'x > 20 gives x'
    v2 = D.view(V['x'])
    D.mish(v2)
    assert torch.equal(D.host(v2).t, h.t), 'two runs differ'


def run_mish_bwd(case, kw, D, rep):
    V = E.mish_views(kw)
    dv = {k: D.view(V[k]) for k in ('x', 'dy', 'dx')}
    sc, sh = kw['scale'], kw['shift']
    D.mish_bwd(dv['x'], dv['dy'], dv['dx'], D.put(sc), D.put(sh))
    h = D.host(dv['dx'])
    got = dense(h).clone()
    x, dy = kw['x'].double(), kw['dy'].double()
    if sc is None:
        assert bool((kw['dy'] == 1).all())
        ref = T.mish_grad(x).float()
        ulps = (got.double() - ref.double()).abs() / _ulp_of(ref)
        i = int(ulps.argmax())
        rep.add('dx', ulps.reshape(-1)[i].item(), 4.0, 4.0)
        rep.notes.append('figures in ulp of the reference')
        assert ulps.max().item() <= 4.0, 'mish backward: %.2f ulp at x = %r' % (ulps.max().item(), kw['x'].reshape(-1)[i].item())
        assert bool((got[kw['x'] > 20] == 1).all()), 'x > 20 gives 1'
    else:
        z = x * sc.double() + sh.double()
        ref = dy * T.mish_grad(z)
        bound = 5.0 * _ulp_of(ref.float()) + dy.abs() * 1.2 * 2.0 ** -23 * ((x * sc.double()).abs() + z.abs())
        err = (got.double() - ref).abs()
        i = int((err / bound).argmax())
        rep.add('dx', err.reshape(-1)[i].item(), bound.reshape(-1)[i].item(), bound.reshape(-1)[i].item())
        assert bool((err <= bound).all()), (err / bound).max().item()
    assert E.outside_untouched(h), 'written outside the slice'
    _refill(dv['dx'])
    D.mish_bwd(dv['x'], dv['dy'], dv['dx'], D.put(sc), D.put(sh))
    assert torch.equal(dense(D.host(dv['dx'])), got), 'two runs differ'
    _untouched(D, dv, V, ('x', 'dy'))


RUNNERS = {'gn_fwd': run_gn_fwd, 'gn_train_bwd': run_gn_train_bwd, 'affine_act_bwd': run_affine_act_bwd, 'mish': run_mish,
           'mish_bwd': run_mish_bwd}


def run_case(case, D, rep=None, kw=None):
    """Build the case and run its op's runner on the adaptor D.  -> the report (filled as far as the runner came, if it raises)."""
    rep = Report(case) if rep is None else rep
    RUNNERS[case.op](case, case.build() if kw is None else kw, D, rep)
    return rep


@pytest.mark.parametrize('name', list(CASES))
def test_norm_act_edge_case(name, capsys):
    rep = Report(CASES[name])
    try:
        run_case(CASES[name], Device(), rep)
    finally:
        with capsys.disabled():
            print('\n' + rep.line())
