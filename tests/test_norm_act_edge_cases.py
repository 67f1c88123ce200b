"""The edge table of tests/norm_act_edge_cases.py is what it says, fair and sharp -- no GPU.  The runners of
tests/test_gpu_norm_act_edges.py are handed CPU stand-ins in place of the kernels: (1) every case keeps its promise (the restated
launch arithmetic reaches the branch the case names, the data are what it claims); (2) fairness: a plain float32 restatement of each
op (two-pass statistics, the formulas of tests/norm_act_train_ref.py) passes every bound the GPU test applies, and a stand-in of the
kernels' own decomposition (shifted double sums per pixel chunk and channel slab, lane-strided combine, float32 apply) passes the
exact statements too; (3) power: a planted fault in that stand-in fails the case that names the branch; (4) every `op` of the table
has a runner and every runner an `op`, and the activation / residual variants cover what the table says they cover."""
import collections

import numpy as np
import pytest
import torch

import norm_act_edge_cases as E
import norm_act_train_ref as T
import test_gpu_norm_act_edges as G
from norm_act_edge_cases import CASES, dense
from ppyolo_hip import ops


def _mish32(v):
    """mish_f32 of csrc/norm_act.h in float32."""
    e = torch.exp(v)
    n = e * (e + 2.0)
    return torch.where(v > 20.0, v, v * (n / (n + 2.0)))


def _act32(u, act):
    return _mish32(u) if act == 'mish' else G._act32(u, act)


def _grad32(u, act):
    """norm_act_grad of csrc/norm_act.h: the sign rule z > 0; Mish in double, rounded once."""
    if act is None:
        return torch.ones_like(u)
    if act == 'mish':
        return T.mish_grad(u.double()).float()
    return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, 0.0 if act == 'relu' else 0.1))


class StandIn(object):
    """The adaptor interface of test_gpu_norm_act_edges.Device on the CPU.  plain=True: the float32 restatement (held to the bounds
    only).  Otherwise the kernels' decomposition as tests/norm_act_edge_cases.py restates the geometry, with an optional fault."""
    FAULTS = ('combine stops after 64 entries', 'last slab dropped', 'dead tail quad read as live', 'blk without the image',
              'one-pass float32 variance', 'raw moments', 'raw moments, clamp removed', 'forward fuses the multiply-add')
    exact = True

    def __init__(self, fault=None, plain=False):
        assert fault is None or fault in self.FAULTS
        self.fault, self.plain, self.exact = fault, plain, not plain

    # -- plumbing --
    def put(self, t):
        return None if t is None else t.clone()

    def view(self, v):
        return None if v is None else ops.View(v.t.clone(), v.coff, v.C)

    host = view

    def get(self, t):
        return t.clone()

    def stats(self, n):
        return torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float32)

    # -- arithmetic --
    def _z(self, xh, ga, be, forward):
        if forward and self.fault == 'forward fuses the multiply-add':
            return (xh.double() * ga.double() + be.double()).float()          # one rounding (the product of two floats is exact in double)
        return xh * ga + be

    def _chunk_sums(self, vals, rows_per, nchunks):
        """vals [P, C] double -> [nchunks, C]: the pixel tree of a workgroup (in double the order of additions is not visible)."""
        out = torch.zeros(nchunks, vals.shape[1], dtype=torch.float64)
        out.index_add_(0, torch.arange(vals.shape[0]) // rows_per, vals)
        return out

    def _group_sums(self, chan, geo, G, weight=None):
        """chan [nchunks, C] -> [nchunks, G]: the channel loop of a workgroup's group threads, per slab."""
        w = chan if weight is None else chan * weight.double()
        out = w.reshape(chan.shape[0], G, -1).sum(2)
        if self.fault == 'dead tail quad read as live' and geo['live_last'] < geo['TX']:
            out[:, -1] += w[:, -4:].sum(1)          # a lane past the last quad counted again
        if self.fault == 'last slab dropped' and geo['slabs'] > 1:
            out[:, (geo['slabs'] - 1) * geo['groups_per_slab']:] = 0.0          # (what the workspace held)
        return out

    def _gn_stats(self, x, G, eps):
        """x [N, P, C] float32 -> mean [N * G] float64, rstd [N * G] float32."""
        N, P, C = x.shape
        cpg = C // G
        xg = x.reshape(N, P, G, cpg).permute(0, 2, 1, 3).reshape(N, G, -1)
        if self.plain:
            mean = xg.mean(2, keepdim=True)
            var = ((xg - mean) ** 2).mean(2)
            return mean.reshape(-1).double(), (1.0 / torch.sqrt(var + eps)).reshape(-1)
        geo = E.gn_geometry(N, 1, P, C, G)
        mean, rstd = torch.zeros(N * G, dtype=torch.float64), torch.zeros(N * G)
        count = float(P * cpg)
        for n in range(N):
            k = x[n, 0, ::cpg].double()                              # the group's shift: its first element
            d = x[n].double() - k.repeat_interleave(cpg)
            a = self._group_sums(self._chunk_sums(d, geo['rows_per'], geo['nchunks']), geo, G).sum(0)
            b = self._group_sums(self._chunk_sums(d * d, geo['rows_per'], geo['nchunks']), geo, G).sum(0)
            m = a / count
            var = b / count - m * m
            if self.fault in ('raw moments', 'raw moments, clamp removed'):
                var = torch.tensor([E.raw_group_var(xg[n, g]) for g in range(G)], dtype=torch.float64)
            if self.fault != 'raw moments, clamp removed':
                var = var.clamp_min(0.0)
            if self.fault == 'one-pass float32 variance':
                m32 = xg[n].mean(1)
                var = ((xg[n] * xg[n]).mean(1) - m32 * m32).clamp_min(0.0).double()
            mean[n * G:(n + 1) * G] = k + m
            rstd[n * G:(n + 1) * G] = (1.0 / torch.sqrt(var + float(np.float32(eps)))).float()
        return mean, rstd

    def _xhat(self, x, mean, rstd, G):
        N, H, W, C = x.shape
        cpg = C // G
        mu = mean.reshape(N, 1, 1, G).repeat_interleave(cpg, dim=3)
        rs = rstd.reshape(N, 1, 1, G).repeat_interleave(cpg, dim=3)
        return (x.double() - mu).float() * rs, rs

    # -- GroupNorm --
    def _gn_forward(self, x, g, b, groups, eps, y, act, res, up=False):
        X = dense(x)
        N, H, W, C = X.shape
        if self.plain:
            r = T.gn_fwd_bwd(G._nchw(X), g, b, groups, act, torch.zeros(N, C, H, W), None if res is None else G._nchw(dense(res)), None, eps)
            out, mean, rstd = r['y'].permute(0, 2, 3, 1), None, None
        else:
            mean, rstd = self._gn_stats(X.reshape(N, H * W, C), groups, eps)
            xh, _ = self._xhat(X, mean, rstd, groups)
            u = self._z(xh, g, b, True)
            if res is not None:
                u = u + dense(res)
            out = _act32(u, act)
        if up:
            out = out.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        dense(y).copy_(out)
        return mean, rstd

    def group_norm(self, x, g, b, groups, eps, y, act, res, upsample2x=False):
        self._gn_forward(x, g, b, groups, eps, y, act, res, upsample2x)

    def group_norm_train(self, x, g, b, groups, eps, y, mean, rstd, act, res):
        m, r = self._gn_forward(x, g, b, groups, eps, y, act, res)
        if m is not None:
            mean.copy_(m)
            rstd.copy_(r)

    def group_norm_bwd(self, x, mean, rstd, g, b, groups, dy, dx, act, res, dz, dgamma, dbeta, train=True):
        X, DY = dense(x), dense(dy)
        N, H, W, C = X.shape
        if self.plain:
            r = T.gn_fwd_bwd(G._nchw(X), g, b, groups, act, G._nchw(DY), None if res is None else G._nchw(dense(res)))
            dense(dx).copy_(r['dx'].permute(0, 2, 3, 1))
            dense(dz).copy_(r['dz'].permute(0, 2, 3, 1))
            if train:
                dgamma.copy_(r['dgamma'])
                dbeta.copy_(r['dbeta'])
            return
        geo = E.gn_geometry(N, H, W, C, groups)
        nch, P, cpg = geo['nchunks'], H * W, C // groups
        xh, rs = self._xhat(X, mean, rstd, groups)
        u = self._z(xh, g, b, False)
        if res is not None:
            u = u + dense(res)
        DZ = DY * _grad32(u, act)
        pc = torch.zeros(N * nch, C, 2, dtype=torch.float64)          # the workspace, as the partial kernel leaves it
        pg = torch.zeros(N * nch, groups, 2, dtype=torch.float64)
        for n in range(N):
            blk = slice(0, nch) if self.fault == 'blk without the image' else slice(n * nch, (n + 1) * nch)
            s = self._chunk_sums(DZ[n].reshape(P, C).double(), geo['rows_per'], nch)
            ss = self._chunk_sums(DZ[n].reshape(P, C).double() * xh[n].reshape(P, C).double(), geo['rows_per'], nch)
            pc[blk, :, 0], pc[blk, :, 1] = s, ss
            pg[blk, :, 0], pg[blk, :, 1] = self._group_sums(s, geo, groups, g), self._group_sums(ss, geo, groups, g)
        stop = 64 if self.fault == 'combine stops after 64 entries' else 1 << 30          # lanes l, l + 64, ...: the loop's later trips
        count = float(P * cpg)
        ab = torch.stack([pg[n * nch:(n + 1) * nch][:stop].sum(0) for n in range(N)]) / count          # [N, G, 2]
        A = ab[..., 0].reshape(N, 1, 1, groups).repeat_interleave(cpg, dim=3)
        B = ab[..., 1].reshape(N, 1, 1, groups).repeat_interleave(cpg, dim=3)
        dense(dx).copy_((rs.double() * (g.double() * DZ.double() - A - xh.double() * B)).float())
        dense(dz).copy_(DZ)
        if train:
            tot = pc[:stop].sum(0)
            dbeta.copy_(tot[:, 0].float())
            dgamma.copy_(tot[:, 1].float())

    # -- AffineChannel --
    def _af_z(self, x, w, b, res, forward):
        u = self._z(dense(x), w, b, forward)
        return u if res is None else u + dense(res)

    def affine_act(self, x, w, b, y, act, res):
        if self.plain:
            r = T.af_fwd_bwd(G._nchw(dense(x)), w, b, act, torch.zeros_like(G._nchw(dense(x))), None if res is None else G._nchw(dense(res)))
            dense(y).copy_(r['y'].permute(0, 2, 3, 1))
            return
        dense(y).copy_(_act32(self._af_z(x, w, b, res, True), act))

    def affine_bwd(self, x, w, b, dy, dx, act, res, dz, dw, db, train=True):
        X, DY = dense(x), dense(dy)
        N, H, W, C = X.shape
        if self.plain:
            r = T.af_fwd_bwd(G._nchw(X), w, b, act, G._nchw(DY), None if res is None else G._nchw(dense(res)))
            dense(dx).copy_(r['dx'].permute(0, 2, 3, 1))
            dense(dz).copy_(r['dz'].permute(0, 2, 3, 1))
            if train:
                dw.copy_(r['dgamma'])
                db.copy_(r['dbeta'])
            return
        geo = E.af_geometry(N, H, W, C)
        DZ = DY * _grad32(self._af_z(x, w, b, res, False), act)
        dense(dx).copy_(DZ * w)
        dense(dz).copy_(DZ)
        if train:
            flat = DZ.reshape(-1, C).double()
            s = self._chunk_sums(flat, geo['rows_per'], geo['nchunks'])
            ss = self._chunk_sums(flat * X.reshape(-1, C).double(), geo['rows_per'], geo['nchunks'])
            stop = 64 if self.fault == 'combine stops after 64 entries' else 1 << 30
            db.copy_(s[:stop].sum(0).float())
            dw.copy_(ss[:stop].sum(0).float())

    # -- Mish --
    def mish(self, v):
        dense(v).copy_(_mish32(dense(v).clone()))

    def mish_bwd(self, x, dy, dx, scale, shift):
        z = dense(x)
        if scale is not None:
            z = z * scale + shift
        dense(dx).copy_(dense(dy) * T.mish_grad(z.double()).float())


def _twin_kw(kw):
    """The case on its twin input: what the plain float32 restatement is asked to do where the original has a mean near 1000."""
    kw = dict(kw, x=kw['twin'])
    del kw['twin']
    kw['value'] = None
    return kw


# ---- (1) promises ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_case_keeps_its_promise(name):
    case = CASES[name]
    kw = case.build()
    case.promise(kw)
    assert case.why and case.op in E.OPS
    for k, v in kw.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert bool(torch.isfinite(v).all()), k
    kw2 = case.build()          # a case is the same data every time it is built
    assert all(torch.equal(v, kw2[k]) for k, v in kw.items() if torch.is_tensor(v))


def test_geometry_restatement_on_the_shapes_of_the_direct_tests():
    """The restatement against the comments of tests/test_gpu_norm_act.py / _train.py, which were read off the kernels' launches."""
    g = E.gn_geometry(2, 70, 70, 32, 4)
    assert (g['nchunks'], g['rows_per']) == (126, 39)
    assert E.gn_geometry(2, 13, 11, 64, 32)['nchunks'] == 5
    assert E.gn_geometry(3, 3, 3, 2048, 32)['slabs'] == 8 and E.gn_geometry(2, 19, 19, 256, 32)['nchunks'] == 12
    assert E.gn_geometry(1, 40, 40, 96, 32)['slabs'] == 1 and E.gn_geometry(1, 40, 40, 96, 32)['TX'] == 32
    assert E.GN_MAX_CHUNKS == 128 and E.af_geometry(3, 40, 40, 32)['nchunks'] == 150


def test_every_unreached_branch_has_a_case():
    """What no direct test reaches, and the case (by its promise) that does."""
    geos = {n: E.gn_geometry(*(kw['shape'] + (kw['groups'],))) for n, kw in ((n, c.build()) for n, c in CASES.items() if c.op == 'gn_train_bwd')}
    some = lambda pred: any(pred(g) for g in geos.values())
    assert some(lambda g: g['group_entries'] > 64) and some(lambda g: g['channel_entries'] > 128)          # the combine's second and third trip
    assert some(lambda g: g['nchunks'] == E.GN_MAX_CHUNKS and g['last_chunk'] == 32) and some(lambda g: g['rows_per'] > 32)
    assert some(lambda g: g['slabs'] == 1 and g['passes'] > 1 and g['live_last'] < 64)                       # 256 < C <= 2048 without slabs
    assert some(lambda g: g['slabs'] > 1 and g['live_last'] < 64) and some(lambda g: g['slabs'] > 1 and g['groups_per_slab'] == 1)
    assert some(lambda g: g['cpg'] == 10) and some(lambda g: g['cpg'] == 1) and some(lambda g: g['TX'] == 1)
    afs = [E.af_geometry(*c.build()['shape']) for c in CASES.values() if c.op == 'affine_act_bwd']
    assert any(a['nchunks'] == E.AF_MAX_CHUNKS for a in afs) and any(a['rows_per'] > 32 for a in afs)
    assert any(a['slabs'] == 2 and a['live_last'] < 64 for a in afs)
    values = collections.Counter(c.build()['value'] for c in CASES.values() if c.op in ('gn_train_bwd', 'affine_act_bwd'))
    assert values['large_mean'] == 2 and values['constant_group'] == 2 and values['zero_preactivation'] == 4 and values['mish_tails'] == 2
    assert values['image_independence'] == 1 and values['slope'] == 6


def test_variants_cover_every_activation_and_residual_per_geometry_class():
    seen = collections.defaultdict(set)
    for shape, _, _, variants in E.GN_GEOMETRY:
        for act, res in variants:
            seen[E.geometry_class(*shape)].update([('act', act), ('res', res)])
    want = set(('act', a) for a in E.ACTS) | set([('res', True), ('res', False)])
    for cls in ('slabbed', 'multi-pass', 'many-chunk'):
        assert seen[cls] == want, (cls, want - seen[cls])


def test_every_op_has_a_runner_and_every_runner_an_op():
    used = set(c.op for c in CASES.values())
    assert used == set(E.OPS) == set(G.RUNNERS), (used, set(G.RUNNERS))
    assert G.K_GN == 3.0 and G.ULP == 2.0 ** -24          # the factors of tests/test_gpu_norm_act_train.py and tests/test_gpu_norm_act.py
    assert set(m for m in dir(G.Device) if not m.startswith('_')) == set(m for m in dir(StandIn) if not m.startswith('_') and m != 'FAULTS')


# ---- (2) fairness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in CASES if not n.startswith('slope_consistency')])
def test_float32_restatement_passes_every_bound(name):
    """The plain float32 restatement, on the twin where the case has one (the restatement is no yardstick for a mean near 1000).
    The sign-pattern cases are exact statements about two kernels and have no bound of their own: the stand-in below runs them."""
    case = CASES[name]
    kw = case.build()
    rep = G.run_case(case, StandIn(plain=True), kw=_twin_kw(kw) if 'twin' in kw else kw)
    assert rep.items and all(err <= bound for _, err, _, bound in rep.items)


@pytest.mark.parametrize('name', list(CASES))
def test_stand_in_of_the_kernels_passes_every_statement(name):
    """Bounds and exact statements: a float32 implementation with the kernels' decomposition can do all that is asked."""
    rep = G.run_case(CASES[name], StandIn())
    assert all(err <= bound for _, err, _, bound in rep.items)
    if CASES[name].build()['value'] == 'slope':
        assert rep.slope['zero'] == rep.slope['chosen'], 'without contraction z is exactly 0 at every chosen element'


# ---- (3) power ---------------------------------------------------------------------------------------------------------------
POWER = [
    ('combine stops after 64 entries', 'gn_train_bwd_2x47x47x32_g8_relu_res'),
    ('combine stops after 64 entries', 'gn_train_bwd_1x64x64x16_g4_leaky'),
    ('combine stops after 64 entries', 'gn_train_bwd_1x70x70x8_g2_none_res'),
    ('combine stops after 64 entries', 'affine_4x64x64x8_relu_res'),
    ('combine stops after 64 entries', 'affine_5x60x60x8_leaky'),
    ('last slab dropped', 'gn_fwd_2x5x7x320_g5_leaky_res'),
    ('last slab dropped', 'gn_train_bwd_2x5x7x320_g5_mish'),
    ('last slab dropped', 'gn_train_bwd_1x3x3x768_g3_none'),
    ('last slab dropped', 'gn_fwd_1x3x3x2048_g8_relu'),
    ('dead tail quad read as live', 'gn_fwd_2x5x7x320_g32_relu'),
    ('dead tail quad read as live', 'gn_train_bwd_2x5x7x320_g32_leaky_res'),
    ('dead tail quad read as live', 'gn_train_bwd_1x2x3x2044_g7_none'),
    ('dead tail quad read as live', 'gn_fwd_2x6x6x40_g4_leaky'),
    ('dead tail quad read as live', 'gn_train_bwd_2x1x33x12_g3_relu'),
    ('blk without the image', 'gn_train_bwd_2x47x47x32_g8_relu_res'),
    ('blk without the image', 'image_independence'),
    ('one-pass float32 variance', 'large_mean_64c_g32'),
    ('one-pass float32 variance', 'large_mean_320c_g5'),
    ('raw moments, clamp removed', 'constant_group_64c_g32'),
    ('raw moments, clamp removed', 'constant_group_320c_g5'),
    ('raw moments, clamp removed', 'zero_preactivation_relu_64c_g32'),
]


@pytest.mark.parametrize('fault,name', POWER)
def test_planted_fault_fails_the_named_case(fault, name):
    with pytest.raises(AssertionError):
        G.run_case(CASES[name], StandIn(fault))


@pytest.mark.parametrize('name', [n for n in CASES if n.startswith(('constant_group', 'zero_preactivation'))])
def test_the_clamp_is_what_the_constant_group_needs(name):
    """The kernels' shifted sums give var == 0 exactly on a constant group, so the clamp is out of reach there; it is what stands
    between a kernel that sums raw moments and a wrong rstd.  Raw double moments WITH the clamp pass the case (the promise picked a
    constant on which they go negative); without it they fail (test_planted_fault_fails_the_named_case)."""
    G.run_case(CASES[name], StandIn('raw moments'))
    with pytest.raises(AssertionError):
        G.run_case(CASES[name], StandIn('raw moments, clamp removed'))


@pytest.mark.parametrize('name', [n for n in CASES if n.startswith('slope_consistency')])
def test_a_forward_that_fuses_beside_a_backward_that_does_not_is_caught(name):
    rep = G.Report(CASES[name])
    with pytest.raises(AssertionError):
        G.run_case(CASES[name], StandIn('forward fuses the multiply-add'), rep)
    s = rep.slope
    print(rep.line())
    assert s['disagree_chosen'] * 4 >= s['chosen'], s
    assert s['pos'] > 0 and s['neg'] > 0 and s['disagree_chosen'] == s['pos'], s


def test_rounding_residual_of_a_product_is_almost_never_zero():
    """What the sign-pattern cases rest on: fma(a, b, -fl(a * b)) is the rounding residual of the product, positive about as often
    as negative and zero for (nearly) no pair of random floats."""
    rng = np.random.RandomState(0)
    a, b = rng.randn(100000).astype(np.float32), (rng.rand(100000) + 0.5).astype(np.float32)
    r = a.astype(np.float64) * b.astype(np.float64) - (a * b).astype(np.float64)
    pos, neg, zero = (r > 0).mean(), (r < 0).mean(), (r == 0).mean()
    print('residual > 0: %.3f, < 0: %.3f, == 0: %.5f' % (pos, neg, zero))
    assert 0.45 < pos < 0.55 and 0.45 < neg < 0.55 and zero < 1e-3
