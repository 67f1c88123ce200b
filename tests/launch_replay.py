"""Launch-level oracle of the training step: every kernel launch of a real TrainStep judged, on the inputs it actually received,
against float64 (test support, like tests/train_parity_util.py).

ppyolo_hip/train.py calls its kernels only through the module attribute `K.<op>` (`from . import ops as K`), so replacing the
attributes of `ppyolo_hip.ops` intercepts every launch.  Per intercepted call the wrapper synchronises, snapshots the inputs and
the WHOLE backing tensor of every output View, runs the real op, synchronises again, computes the float64 reference and checks
it, then frees the snapshots.  Because the reference starts from what the kernel itself was given, the chaos of a training-mode
network (batch statistics, activation slopes, upstream rounding) is out of the comparison: the tolerance is set by rounding alone,
per element.

Contractions (forward convolutions, data / weight gradients, the stem) are referenced as per-tap shifted GEMMs in float64 on the
device -- no F.conv2d -- and held to

    |got - ref| <= C_BOUND * [(u_fmt + 2^-24 sqrt(k)) sqrt(sum A^2 B^2) + u_floor floor(A, B) + 2^-24 |ref|]

k: reduction length; u_fmt: 2^-22 for the split (f16x2 / bf16x3) kernels, 2^-24 for exact-fp32 MFMA and fma chains; u_floor: 2^-36
on the f16x2 kernels -- second terms of an operand scaled by its per-image (activations, gradients) or per-channel (weights) maximum
underflow fp16 below that -- with floor = amax_n(A) sum|B| + amax_k(B) sum|A| over the taps; the last term is the fp32 rounding of
the output itself (bias / scale in the epilogue).  The bound is statistical on purpose: the worst case k 2^-24 |A||B| is ~1000x
looser at k = 9216 and would not see a dropped 32-channel chunk.  C_BOUND is one constant for every contraction.

Everything else is a float64 formula with a bound of a few ulps (C_BOUND 2^-24 per rounding), and for reductions over P terms
C_BOUND 2^-24 (|S| + sqrt(P) sqrt(sum t^2)).

Tracked maxima (ops.amax_slots blocks): an op that writes the maximum of its OWN output (bn_train_apply, bn_train_bwd,
conv1x1_bn_apply, yolov3_loss's dout) must make max(block) == max(before, max|output of image n|) exactly (rule 'exact').

Writes outside a View's slice: every byte of an output's backing tensor outside the union of the call's output slices must be
bit-identical before and after the call.
"""
import collections
import inspect
import math

import torch
import torch.nn.functional as F

C_BOUND = 8.0
U24 = 2.0 ** -24
U22 = 2.0 ** -22
U_FLOOR_F16 = 2.0 ** -36
AMAX_PER_IMAGE = 128

# Ops the replay does not judge numerically, with the reason; the test asserts that every op a step calls is either checked or
# listed here, so an op added to ppyolo_hip/ops.py cannot escape silently.
ALLOWLIST = {
    'dropblock_mask': 'random draw: structure only (values 0 / 1, scale = numel / sum(mask))',
    'split_weights_f16x2': 'operand re-encoding of a weight; every convolution that reads the planes is checked against the fp32 master',
    'split_weights_bf16x3': 'operand re-encoding of a weight; as split_weights_f16x2',
    'WeightPrepTable': 'operand re-encoding of the trainable weights; the prepared data gradients are checked against the fp32 master',
    'amax_slots': 'torch reduction (no kernel): the maximum its consumer is scaled by',
}
# host-only helpers and types: no launch
HOST = {'View', 'conv_out_hw', 'dcn_out_hw', 'conv2d_workspace_bytes', 'conv2d_pick', 'ConvCfg', 'conv_cfg', 'conv_cfgs', 'stream_first_cfg', 'ws_first_cfg',
        'small_first_cfg', 'patch_first_cfg', 'conv2d_bn_partials_bytes', 'dcnv2_num_configs', 'dcnv2_scheme',
        'dcnv2_configs', 'dcnv2_workspace_bytes', 'matrix_nms_workspace'}


class ReplayFailure(AssertionError):
    pass


# ---- helpers -------------------------------------------------------------------------------------------------------------
def dense64(v):
    return v.t[..., v.coff:v.coff + v.C].double()


def slope_of(y, act):
    """d act / d z from the OUTPUT (the kernels' rule: y > 0 <=> pre-activation > 0), float64."""
    if act is None:
        return torch.ones_like(y, dtype=torch.float64)
    neg = 0.0 if act == 'relu' else 0.1
    return torch.where(y > 0, torch.ones_like(y, dtype=torch.float64), torch.full_like(y, neg, dtype=torch.float64))


def amax_per_image(block, N):
    """max over an amax_slots block per image -> [N] float64."""
    return block.view(N, AMAX_PER_IMAGE).double().amax(dim=1)


def _pad_nhwc(x, pad):
    return F.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x


def conv_taps(x, w, stride, pad, Ho=None, Wo=None):
    """y[n, ho, wo, k] = sum_{r,s,c} x[n, ho*stride + r - pad, wo*stride + s - pad, c] w[k, r, s, c]: x NHWC, w KRSC, float64, one
    GEMM per tap (zero padding)."""
    N, H, W, C = x.shape
    K, R, S, C2 = w.shape
    assert C == C2
    Ho = (H + 2 * pad - R) // stride + 1 if Ho is None else Ho
    Wo = (W + 2 * pad - S) // stride + 1 if Wo is None else Wo
    xp = _pad_nhwc(x, pad)
    y = torch.zeros((N * Ho * Wo, K), dtype=torch.float64, device=x.device)
    for r in range(R):
        for s in range(S):
            xs = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :].reshape(-1, C)
            y += xs @ w[:, r, s, :].t()
    return y.view(N, Ho, Wo, K)


def conv_reference(x, w, stride, pad, amax_x=None):
    """-> (ref, sqrt(sum A^2 B^2), floor) of a forward convolution, all float64 [N, Ho, Wo, K].  amax_x: [N] operand scale."""
    ref = conv_taps(x, w, stride, pad)
    sq = conv_taps(x * x, w * w, stride, pad).clamp_min(0).sqrt()
    N = x.shape[0]
    ax = x.abs().reshape(N, -1).amax(dim=1) if amax_x is None else torch.maximum(amax_x, x.abs().reshape(N, -1).amax(dim=1))
    wabs = w.abs()
    floor = ax.view(N, 1, 1, 1) * wabs.reshape(w.shape[0], -1).sum(dim=1).view(1, 1, 1, -1)
    xsum = conv_taps(x.abs(), torch.ones((1,) + tuple(w.shape[1:]), dtype=torch.float64, device=x.device), stride, pad)
    floor = floor + xsum * wabs.reshape(w.shape[0], -1).amax(dim=1).view(1, 1, 1, -1)
    return ref, sq, floor


def dgrad_weight(w):
    """KRSC weight -> the flipped / transposed one the data gradient convolves with: w'[c, r, s, k] = w[k, R-1-r, S-1-s, c]."""
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def contraction_bound(ref, sq, floor, k, u_fmt, u_floor):
    return C_BOUND * ((u_fmt + U24 * math.sqrt(k)) * sq + u_floor * floor + U24 * ref.abs())


def sum_bound(S, t, P):
    """C_BOUND 2^-24 (|S| + sqrt(P) sqrt(sum t^2)) of a reduction S = sum over P terms t (t reduced over dim 0)."""
    return C_BOUND * U24 * (S.abs() + math.sqrt(P) * (t * t).sum(dim=0).sqrt())


# ---- conv families -------------------------------------------------------------------------------------------------------
def conv_family(ops, cfg, f16, x3):
    """Kernel family a conv cfg id selects (ops.conv_cfg; the f16x2 tile kinds and the two plain kinds of specialised-wave tiles as one each)."""
    if cfg is None or cfg < 0:
        return 'default-f16x2' if f16 else ('default-bf16x3' if x3 else 'default-fp32')
    fam = ops.conv_cfg(cfg).family
    return {'f16x2_slab': 'f16x2', 'f16x2_tall': 'f16x2', 'ws_pre': 'ws'}.get(fam, fam)


def family_units(fam, f16):
    """(u_fmt, u_floor) of a conv family."""
    if fam in ('fp32', 'default-fp32'):
        return U24, 0.0
    return U22, (U_FLOOR_F16 if f16 else 0.0)


# ---- the interceptor -----------------------------------------------------------------------------------------------------
class Replay(object):
    """Install with `install(monkeypatch)`; after the step, `census` holds one record per launch, `failures` the launches out of
    bound, `unchecked` the ops called without a reference (op -> count)."""

    def __init__(self, ops, ts=None, verbose=False):
        self.ops = ops
        self.ts = ts                   # TrainStep: weights behind f16x2 planes (conv1x1_stats / conv1x1_bn_apply read planes only)
        self.census = []
        self.failures = []
        self.unchecked = collections.Counter()
        self.declined = []
        self.verbose = verbose
        self.orig = {}
        self._cur = None

    # -- installation
    def install(self, monkeypatch):
        for name, fn in list(vars(self.ops).items()):
            if name.startswith('_') or name in HOST:
                continue
            if not (inspect.isfunction(fn) or inspect.isclass(fn)) or getattr(fn, '__module__', None) != self.ops.__name__:
                continue
            self.orig[name] = fn
            monkeypatch.setattr(self.ops, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        chk = getattr(self, 'chk_' + name, None)
        if inspect.isclass(fn):
            def cls_wrapper(*a, **kw):
                self.unchecked[name] += 1
                return fn(*a, **kw)
            return cls_wrapper
        sig = inspect.signature(fn)

        def wrapper(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            if chk is None:
                self.unchecked[name] += 1
                return fn(*a, **kw)
            return self.run(name, dict(ba.arguments), lambda: fn(*a, **kw))
        return wrapper

    @staticmethod
    def bind(fn, *a, **kw):
        """The argument dict a checker receives for the call fn(*a, **kw) (defaults applied)."""
        ba = inspect.signature(fn).bind(*a, **kw)
        ba.apply_defaults()
        return dict(ba.arguments)

    def run(self, name, args, call):
        """Check one launch: `call()` runs the real op; `args` its bound arguments."""
        chk = getattr(self, 'chk_' + name)
        sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)
        sync()
        self._cur = dict(op=name, checks=[], meta={})
        try:
            with torch.no_grad():
                out = chk(args, call)
        except Exception as e:
            from ppyolo_hip._lib import PPYoloHipError
            if isinstance(e, PPYoloHipError):
                self.declined.append(dict(op=name, error=str(e), **self._cur['meta']))
            self._cur = None
            raise
        sync()
        rec = dict(op=name, **self._cur['meta'])
        rec['ratio'] = max([c[1] for c in self._cur['checks']] + [0.0])
        rec['checks'] = [c[0] for c in self._cur['checks']]
        self.census.append(rec)
        self._cur = None
        return out

    # -- recording
    def meta(self, **kw):
        self._cur['meta'].update(kw)

    def compare(self, what, got, ref, bound):
        """Elementwise |got - ref| <= bound (float64); records the worst ratio of the current launch."""
        got = got.double()
        err = (got - ref).abs()
        bad_nan = torch.isnan(got) & ~torch.isnan(ref)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        ratio = torch.where(bad_nan, torch.full_like(ratio, math.inf), ratio)
        ratio = torch.nan_to_num(ratio, nan=0.0, posinf=math.inf)
        worst = float(ratio.max()) if ratio.numel() else 0.0
        self._cur['checks'].append((what, worst))
        if not worst <= 1.0:
            i = int(ratio.reshape(-1).argmax())
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape)) if ratio.dim() else ()
            self.failures.append(dict(op=self._cur['op'], what=what, index=idx, got=float(got.reshape(-1)[i]), ref=float(ref.reshape(-1)[i]),
                                      bound=float(bound.reshape(-1)[i]) if bound.dim() else float(bound), ratio=worst,
                                      bad=int((ratio > 1).sum()), **self._cur['meta']))
        return worst

    def exact(self, what, got, ref):
        ok = torch.equal(got, ref)
        self._cur['checks'].append((what, 0.0 if ok else math.inf))
        if not ok:
            d = (got.double() - ref.double()).abs()
            i = int(torch.nan_to_num(d, nan=math.inf).reshape(-1).argmax())
            self.failures.append(dict(op=self._cur['op'], what=what, index=i, got=float(got.reshape(-1)[i]), ref=float(ref.reshape(-1)[i]),
                                      ratio=math.inf, bad=int((got != ref).sum()), **self._cur['meta']))

    def fail(self, what, **info):
        self._cur['checks'].append((what, math.inf))
        self.failures.append(dict(op=self._cur['op'], what=what, ratio=math.inf, **info, **self._cur['meta']))

    # -- output snapshots: the whole backing tensor, the slices the call may write
    def snap_out(self, *views):
        groups = collections.OrderedDict()
        for v in views:
            if v is None:
                continue
            key = (v.t.data_ptr(), tuple(v.t.shape))
            groups.setdefault(key, [v.t, v.t.clone(), []])[2].append((v.coff, v.C))
        return list(groups.values())

    def check_outside(self, snaps):
        for t, before, spans in snaps:
            keep = torch.ones(t.shape[-1], dtype=torch.bool, device=t.device)
            for coff, C in spans:
                keep[coff:coff + C] = False
            if bool(keep.any()):
                a, b = t[..., keep], before[..., keep]
                if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
                    bad = (a.view(torch.int32) != b.view(torch.int32)).nonzero()[0].tolist()
                    chans = keep.nonzero().view(-1)
                    self.fail('write outside the slice', index=bad[:-1] + [int(chans[bad[-1]])], spans=spans)
                else:
                    self._cur['checks'].append(('outside slice', 0.0))

    def before_slice(self, snaps, v):
        for t, before, _ in snaps:
            if t.data_ptr() == v.t.data_ptr():
                return before[..., v.coff:v.coff + v.C].double()
        raise KeyError('no snapshot')

    def check_amax_exact(self, block, before, out_dense):
        N = out_dense.shape[0]
        want = torch.maximum(amax_per_image(before, N), out_dense.abs().reshape(N, -1).amax(dim=1).double())
        self.exact('amax (exact)', amax_per_image(block, N), want)

    def weight_of_planes(self, planes):
        """The fp32 KRSC master behind an f16x2 plane pair (the TrainStep's weight cache)."""
        if self.ts is not None:
            for ent in self.ts._wcache.values():
                f = ent.get('f16')
                if f is not None and f[0].data_ptr() == planes.data_ptr():
                    return ent['krsc']
        raise ReplayFailure('no fp32 master found for an f16x2 weight plane pair')

    # ---- contractions ------------------------------------------------------------------------------------------------
    def _conv_check(self, x, w, stride, pad, amax, fam, f16, got, scale=None, shift=None, res=None, act_y=None, act=None, shift_mag=None):
        """Forward conv reference y = act(conv * scale + shift + res) with the slope locked to the kernel's own y."""
        amax_n = None if amax is None else amax_per_image(amax, x.shape[0])
        ref, sq, floor = conv_reference(x, w, stride, pad, amax_n)
        u_fmt, u_floor = family_units(fam, f16)
        k = w.shape[1] * w.shape[2] * w.shape[3]
        bound = contraction_bound(ref, sq, floor, k, u_fmt, u_floor)
        if scale is not None:
            ref = ref * scale.double().view(1, 1, 1, -1)
            bound = bound * scale.double().abs().view(1, 1, 1, -1)
        if shift is not None:
            ref = ref + shift.double().view(1, 1, 1, -1)
            bound = bound + C_BOUND * U24 * (shift.double().abs() if shift_mag is None else shift_mag).view(1, 1, 1, -1)
        if res is not None:
            ref = ref + res
            bound = bound + C_BOUND * U24 * (res.abs() + ref.abs())
        if act is not None:
            sl = slope_of(act_y, act)
            ref, bound = ref * sl, bound * sl.abs().clamp_min(0.1)
        self.compare('conv (k=%d)' % k, got, ref, bound)
        return ref

    def chk_conv2d_bn_act(self, a, call):
        x, w, y = a['x'], a['w_krsc'], a['y']
        assert a['x_split'] is None and a['y_split'] is None and not a['upsample2x'] and a['posbias'] is None
        f16 = a['w_f16'] is not None and a['amax_in'] is not None
        fam = conv_family(self.ops, a['cfg'], f16, a['w_x3'] is not None)
        self.meta(geom=(x.N, x.H, x.W, x.C, w.shape[0], w.shape[1], a['stride']), cfg=a['cfg'], splitk=a['splitk'], family=fam, kind='fwd')
        xs = dense64(x)
        res = None if a['residual'] is None else dense64(a['residual'])
        snaps = self.snap_out(y)
        amax_before = None if a['amax_out'] is None else a['amax_out'].clone()
        out = call()
        got = dense64(y)
        self._conv_check(xs, w.double(), a['stride'], a['pad'], a['amax_in'], fam, f16, got, a['scale'], a['shift'], res, got, a['act'])
        self.check_outside(snaps)
        if amax_before is not None:
            self.check_amax_exact(a['amax_out'], amax_before, got)
        return out

    def _bn_stats_check(self, mean_ref_src, partials, slices, C):
        """Partials [slices][C][3] = (n, mean, M2) merged in float64 -> (n, mean, var)."""
        p = partials[:slices * C * 3].view(slices, C, 3).double()
        n, m, m2 = p[..., 0], p[..., 1], p[..., 2]
        ntot = n.sum(dim=0)
        mean = (n * m).sum(dim=0) / ntot
        M2 = (m2 + n * (m - mean) ** 2).sum(dim=0)
        return ntot, mean, M2, (n, m, m2)

    def _partials_vs(self, partials, slices, C, y_ref, bound_el):
        """The epilogue's BatchNorm partials against float64 statistics of y_ref (the kernel's own output, or the float64 conv
        with its per-element bound when the output is never stored)."""
        ntot, mean, M2, _ = self._bn_stats_check(None, partials, slices, C)
        yy = y_ref.reshape(-1, C)
        P = yy.shape[0]
        self.exact('partials count', ntot, torch.full_like(ntot, float(P)))
        m_ref = yy.mean(dim=0)
        d = yy - m_ref
        v_ref = (d * d).mean(dim=0)
        b_el = bound_el.reshape(-1, C) if bound_el is not None else torch.zeros_like(yy)
        self.compare('partials mean', mean, m_ref, sum_bound(m_ref * P, yy, P) / P + b_el.mean(dim=0))
        self.compare('partials var', M2 / P, v_ref, sum_bound(v_ref * P, d * d, P) / P + 2 * (d.abs() * b_el).mean(dim=0) + b_el.pow(2).mean(dim=0))

    def chk_conv2d_train_fwd(self, a, call):
        x, w, y = a['x'], a['w_krsc'], a['y']
        fam = conv_family(self.ops, a['cfg'], True, False)
        self.meta(geom=(x.N, x.H, x.W, x.C, w.shape[0], w.shape[1], a['stride']), cfg=a['cfg'], splitk=1, family=fam, kind='fwd')
        xs = dense64(x)
        snaps = self.snap_out(y)
        slices = call()
        got = dense64(y)
        self._conv_check(xs, w.double(), a['stride'], a['pad'], a['amax_in'], fam, True, got, None, a['bias'])
        self.check_outside(snaps)
        self._partials_vs(a['partials'], slices, w.shape[0], got, None)
        return slices

    def chk_conv1x1_stats(self, a, call):
        x = a['x']
        w = self.weight_of_planes(a['w_f16'][0])
        Kout = a['Kout']
        self.meta(geom=(x.N, x.H, x.W, x.C, Kout, 1, 1), cfg=self.ops.stream_first_cfg() + a['variant'], splitk=1, family='stream',
                  kind='fwd-stats')
        xs = dense64(x)
        slices = call()
        amax_n = amax_per_image(a['amax_in'], x.N)
        ref, sq, floor = conv_reference(xs, w.double(), 1, 0, amax_n)
        ref = ref + a['bias'].double().view(1, 1, 1, -1)
        bound = contraction_bound(ref, sq, floor, x.C, U22, U_FLOOR_F16)
        self._partials_vs(a['partials'], slices, Kout, ref, bound)
        return slices

    def chk_conv1x1_bn_apply(self, a, call):
        x, y = a['x'], a['y']
        w = self.weight_of_planes(a['w_f16'][0])
        self.meta(geom=(x.N, x.H, x.W, x.C, y.C, 1, 1), cfg=self.ops.stream_first_cfg() + a['variant'], splitk=1, family='stream',
                  kind='fwd-apply')
        xs = dense64(x)
        res = None if a['residual'] is None else dense64(a['residual'])
        snaps = self.snap_out(y)
        amax_before = None if a['amax_out'] is None else a['amax_out'].clone()
        out = call()
        got = dense64(y)
        g = (a['invstd'].double() * a['gamma'].double())
        # (conv + bias - mean) * (invstd * gamma) + beta: the conv's bound scaled by |invstd * gamma|, and one rounding per step
        shift = a['beta'].double() - (a['mean'].double() - a['bias'].double()) * g
        mag = a['beta'].double().abs() + (a['mean'].double().abs() + a['bias'].double().abs()) * g.abs()
        self._conv_check(xs, w.double(), 1, 0, a['amax_in'], 'stream', True, got, g, shift, res, got, a['act'], shift_mag=mag)
        self.check_outside(snaps)
        if amax_before is not None:
            self.check_amax_exact(a['amax_out'], amax_before, got)
        return out

    def _dgrad(self, a, call, w, stride, pad, prepared):
        dy, dx = a['dy'], a['dx']
        f16 = a['amax_dy'] is not None
        fam = conv_family(self.ops, a['cfg'], f16, not f16)
        K, R, S, C = w.shape
        self.meta(geom=(dx.N, dx.H, dx.W, _r32(K), C, R, 1), cfg=a['cfg'], splitk=a['splitk'], family=fam, kind='dgrad',
                  prepared=prepared)
        dys = dense64(dy)
        snaps = self.snap_out(dx)
        out = call()
        got = dense64(dx)
        amax_n = None if not f16 else amax_per_image(a['amax_dy'], dy.N)
        ref, sq, floor = conv_reference(dys, dgrad_weight(w.double()), 1, R - 1 - pad, amax_n)
        u_fmt, u_floor = family_units(fam, f16)
        self.compare('dgrad (k=%d)' % (R * S * K), got, ref, contraction_bound(ref, sq, floor, R * S * K, u_fmt, u_floor))
        self.check_outside(snaps)
        return out

    def chk_conv2d_dgrad(self, a, call):
        assert a['stride'] == 1
        return self._dgrad(a, call, a['w_krsc'], 1, a['pad'], False)

    def chk_conv2d_dgrad_prepared(self, a, call):
        return self._dgrad(a, call, a['prep']['w'], 1, a['pad'], True)

    def chk_conv2d_wgrad(self, a, call):
        x, dy, dw = a['x'], a['dy'], a['dw_krsc']
        K, R, S, C = dw.shape
        stride, pad = a['stride'], a['pad']
        f16 = a['amax_x'] is not None
        nine = R == 3 and S == 3 and stride == 1 and pad == 1 and C % 32 == 0
        fam = ('wgrad-nine-tap' if nine else 'wgrad-x3') + ('-f16x2' if f16 else '')
        self.meta(geom=(x.N, x.H, x.W, C, K, R, stride), cfg=None, splitk=None, family=fam, kind='wgrad')
        xs, dys = dense64(x), dense64(dy)
        out = call()
        got = dw.double()
        N, Ho, Wo = dy.N, dy.H, dy.W
        xp = _pad_nhwc(xs, pad)
        P = N * Ho * Wo
        d2 = dys.reshape(P, K)
        ref = torch.empty((K, R, S, C), dtype=torch.float64, device=dw.device)
        sq = torch.empty_like(ref)
        floor = torch.zeros_like(ref)
        if f16:
            ax = amax_per_image(a['amax_x'], N).repeat_interleave(Ho * Wo).view(P, 1)
            ad = amax_per_image(a['amax_dy'], N).repeat_interleave(Ho * Wo).view(P, 1)
            fk = (ax * d2.abs()).sum(dim=0)
        for r in range(R):
            for s in range(S):
                xt = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :].reshape(P, C)
                ref[:, r, s, :] = d2.t() @ xt
                sq[:, r, s, :] = (d2 * d2).t() @ (xt * xt)
                if f16:
                    # (a tap / channel whose x is zero at every pixel -- padding only, as the off-centre taps of a 1 x 1 map -- is a sum
                    # of exact zeros whatever the operand scale: no floor, the result must be exactly 0)
                    live = (xt.abs().sum(dim=0) > 0).view(1, C)
                    floor[:, r, s, :] = (fk.view(K, 1) + (xt.abs() * ad).sum(dim=0).view(1, C)) * live
        u_fmt, u_floor = (U22, U_FLOOR_F16) if f16 else (U22, 0.0)
        self.compare('wgrad (k=%d)' % P, got, ref, contraction_bound(ref, sq.clamp_min(0).sqrt(), floor, P, u_fmt, u_floor))
        return out

    def chk_stem_conv(self, a, call):
        x, w, y = a['x_nchw'], a['w_kcrs'], a['y']
        fam = 'stem-bf16x3' if a['mfma'] else 'stem-fp32'
        self.meta(geom=(x.shape[0], x.shape[2], x.shape[3], 3, w.shape[0], 3, 2), cfg=None, splitk=None, family=fam, kind='fwd')
        xs = x.permute(0, 2, 3, 1).double()
        snaps = self.snap_out(y)
        amax_before = None if a['amax_out'] is None else a['amax_out'].clone()
        out = call()
        got = dense64(y)
        self._conv_check(xs, w.permute(0, 2, 3, 1).double(), 2, 1, None, 'fp32' if not a['mfma'] else 'bf16x3', False, got, a['scale'],
                         a['shift'], None, got, a['act'])
        self.check_outside(snaps)
        if amax_before is not None:
            self.check_amax_exact(a['amax_out'], amax_before, got)
        return out

    # ---- DCNv2 ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def dcn_sample(x, om, stride, pad):
        """The modulated bilinear samples of DCNv2 (oracle/ppyolo_oracle.dcnv2_sample) from the launch's own x [N,H,W,C] and RAW
        offset_mask [N,Ho,Wo,27].  Positions, corners and bilinear fractions are computed in fp32 as the reference's arithmetic
        prescribes (the image index folded into the fp32 row coordinate before floor); the blend itself in float64.  Returns a
        dict: cols [P,9,C] (float64), the four corner values and weights, the mask, and which taps were clamped."""
        N, H, W, C = x.shape
        Ho, Wo = om.shape[1], om.shape[2]
        dev = x.device
        Hp, Wp = H + 2 * pad + 1, W + 2 * pad + 1
        xp = torch.zeros((N, Hp, Wp, C), dtype=torch.float64, device=dev)
        xp[:, pad:pad + H, pad:pad + W] = x.double()
        flat = xp.view(N * Hp * Wp, C)
        om32 = om.float()
        oy = (torch.arange(Ho, dtype=torch.float32, device=dev) * stride + pad).view(1, Ho, 1, 1)
        ox = (torch.arange(Wo, dtype=torch.float32, device=dev) * stride + pad).view(1, 1, Wo, 1)
        ty = (torch.arange(3, dtype=torch.float32, device=dev) - 1).view(3, 1).repeat(1, 3).reshape(1, 1, 1, 9)
        tx = (torch.arange(3, dtype=torch.float32, device=dev) - 1).view(1, 3).repeat(3, 1).reshape(1, 1, 1, 9)
        off = om32[..., :18].reshape(N, Ho, Wo, 9, 2)
        py = (oy + ty) + off[..., 0]
        px = (ox + tx) + off[..., 1]
        cy = (py < 0) | (py > H + 2 * pad - 1.0)
        cx = (px < 0) | (px > W + 2 * pad - 1.0)
        py = torch.clamp(py, 0.0, H + 2 * pad - 1.0) + (torch.arange(N, dtype=torch.float32, device=dev) * Hp).view(N, 1, 1, 1)
        px = torch.clamp(px, 0.0, W + 2 * pad - 1.0)
        y1, x1 = torch.floor(py), torch.floor(px)
        lh, lw = (py - y1).double(), (px - x1).double()
        hh, hw = 1 - lh, 1 - lw
        iy, ix = y1.long(), x1.long()
        idx = [(iy * Wp + ix), (iy * Wp + ix + 1), ((iy + 1) * Wp + ix), ((iy + 1) * Wp + ix + 1)]
        v = [flat[i.reshape(-1)].view(N * Ho * Wo, 9, C) for i in idx]
        wts = [(hh * hw), (hh * lw), (lh * hw), (lh * lw)]
        wts = [t.reshape(-1, 9, 1) for t in wts]
        m = torch.sigmoid(om[..., 18:27].double()).reshape(-1, 9, 1)
        raw = sum(wt * vv for wt, vv in zip(wts, v))
        mag = sum(wt * vv.abs() for wt, vv in zip(wts, v))
        return dict(cols=raw * m, raw=raw, mag=mag * m, v=v, w=wts, m=m, idx=[i.reshape(-1, 9) for i in idx], lh=lh.reshape(-1, 9, 1),
                    lw=lw.reshape(-1, 9, 1), clamped_y=cy.reshape(-1, 9), clamped_x=cx.reshape(-1, 9), Hp=Hp, Wp=Wp)

    def chk_dcnv2(self, a, call):
        """DCNv2 forward: the contraction of the sampled columns with w in float64.  The magnitude operand of the bound is |x|
        sampled with the same bilinear weights; the fp32 blend of the four corners adds 4 roundings per column entry."""
        x, w, om, y = a['x'], a['w_krsc'], a['offset_mask'], a['y']
        K = w.shape[0]
        f16 = a['w_f16'] is not None and a['amax_in'] is not None
        fam = 'dcn-' + (self.ops.dcnv2_scheme(a['cfg']) if a['cfg'] is not None and a['cfg'] >= 0 else
                        ('f16x2' if f16 else ('bf16x3' if a['w_x3'] is not None else 'fp32')))
        self.meta(geom=(x.N, x.H, x.W, x.C, K, 3, a['stride']), cfg=a['cfg'], splitk=a['splitk'], family=fam, kind='dcn-fwd')
        s = self.dcn_sample(dense64(x), dense64(om), a['stride'], a['pad'])
        snaps = self.snap_out(y)
        out = call()
        got = dense64(y)
        P = s['cols'].shape[0]
        cols, mag = s['cols'].reshape(P, -1), s['mag'].reshape(P, -1)
        w2 = w.double().reshape(K, -1)
        ref = cols @ w2.t()
        sq = ((cols * cols) @ (w2 * w2).t()).sqrt()
        u_fmt, u_floor = family_units('fp32' if fam == 'dcn-fp32' else 'x', fam == 'dcn-f16x2')
        floor = 0.0
        if fam == 'dcn-f16x2':
            ax = torch.maximum(amax_per_image(a['amax_in'], x.N), dense64(x).abs().reshape(x.N, -1).amax(1))
            floor = ax.repeat_interleave(P // x.N).view(P, 1) * w2.abs().sum(1).view(1, K) + mag.sum(1, keepdim=True) * w2.abs().amax(1).view(1, K)
        k = w2.shape[1]
        bound = contraction_bound(ref, sq, floor if torch.is_tensor(floor) else torch.zeros_like(ref), k, u_fmt, u_floor)
        bound = bound + C_BOUND * 4 * U24 * ((mag * mag) @ (w2 * w2).t()).sqrt()
        sc, sh = a['scale'].double().view(1, K), a['shift'].double().view(1, K)
        ref = ref * sc + sh
        bound = bound * sc.abs() + C_BOUND * U24 * (sh.abs() + ref.abs())
        sl = slope_of(got, a['act']).reshape(P, K)
        self.compare('dcn (k=%d)' % k, got.reshape(P, K), ref * sl, bound * sl.abs().clamp_min(0.1))
        self.check_outside(snaps)
        return out

    def chk_dcnv2_backward(self, a, call):
        """DCNv2 backward from the launch's own x, offset_mask and dy: dcols = dy w (k = K); dw = dy^T cols (k = P); dx = the
        bilinear scatter of dcols * mask; d_offset / d_mask logit = sum over C of dcols times the derivative of the blend.  Taps
        whose position was clamped get EXACTLY zero offset gradient (the clamp's derivative)."""
        x, w, om, dy, dx, dom, dw = a['x'], a['w_krsc'], a['offset_mask'], a['dy'], a['dx'], a['d_offset_mask'], a['dw_krsc']
        K, C = w.shape[0], x.C
        self.meta(geom=(x.N, x.H, x.W, C, K, 3, a['stride']), cfg=None, splitk=None, family='dcn-bwd', kind='dcn-bwd')
        xs = dense64(x)
        s = self.dcn_sample(xs, dense64(om), a['stride'], a['pad'])
        d = dense64(dy)
        snaps = self.snap_out(dx, dom)
        out = call()
        P = d.shape[0] * d.shape[1] * d.shape[2]
        d = d.reshape(P, K)
        w2 = w.double().reshape(K, 9 * C)
        dcols = (d @ w2).view(P, 9, C)
        bdc = C_BOUND * ((U22 + U24 * math.sqrt(K)) * ((d * d) @ (w2 * w2)).sqrt().view(P, 9, C) + U24 * dcols.abs())
        # weight gradient
        cols, mag = s['cols'].reshape(P, -1), s['mag'].reshape(P, -1)
        ref = d.t() @ cols
        bound = C_BOUND * ((U22 + U24 * math.sqrt(P)) * ((d * d).t() @ (cols * cols)).sqrt() + 4 * U24 * ((d * d).t() @ (mag * mag)).sqrt()
                           + U24 * ref.abs())
        self.compare('dcn dw (k=%d)' % P, dw.double().reshape(K, -1), ref, bound)
        # data gradient: scatter into the padded frame, cropped
        N, H, W = x.N, x.H, x.W
        Hp, Wp, pad = s['Hp'], s['Wp'], a['pad']
        m = s['m']
        acc = torch.zeros((N * Hp * Wp, C), dtype=torch.float64, device=d.device)
        bacc = torch.zeros_like(acc)
        for i in range(4):
            c = dcols * m * s['w'][i]
            acc.index_add_(0, s['idx'][i].reshape(-1), c.reshape(-1, C))
            bacc.index_add_(0, s['idx'][i].reshape(-1), (m * s['w'][i] * bdc + 2 * C_BOUND * U24 * c.abs()).reshape(-1, C))
        crop = lambda t: t.view(N, Hp, Wp, C)[:, pad:pad + H, pad:pad + W]
        self.compare('dcn dx', dense64(dx), crop(acc), crop(bacc))
        # offset / mask-logit gradients
        v, lh, lw = s['v'], s['lh'], s['lw']
        vabs = sum(t.abs() for t in v)
        d_lh = (1 - lw) * (v[2] - v[0]) + lw * (v[3] - v[1])          # d blend / d lh
        d_lw = (1 - lh) * (v[1] - v[0]) + lh * (v[3] - v[2])          # d blend / d lw
        dm = m * (1 - m)
        got = dense64(dom).reshape(P, 27)
        for what, deriv, sl, clamped in (('dcn d_offset_y', m * d_lh, slice(0, 18, 2), s['clamped_y']),
                                         ('dcn d_offset_x', m * d_lw, slice(1, 18, 2), s['clamped_x']),
                                         ('dcn d_mask', dm * s['raw'], slice(18, 27), None)):
            t = dcols * deriv
            ref = t.sum(2)
            bound = ((deriv.abs() * bdc).sum(2) + C_BOUND * U24 * (math.sqrt(C) * (t * t).sum(2).sqrt() + ref.abs()
                                                                   + 4 * (dcols.abs() * m * vabs).sum(2)))
            g = got[:, sl]
            if clamped is not None:
                ref, bound = torch.where(clamped, torch.zeros_like(ref), ref), torch.where(clamped, torch.zeros_like(bound), bound)
                if bool((g[clamped] != 0).any()):
                    self.fail(what + ': clamped tap with a non-zero offset gradient')
            self.compare(what, g, ref, bound)
        self.check_outside(snaps)
        return out

    # ---- BatchNorm -----------------------------------------------------------------------------------------------------
    def _stats_outputs(self, a, mean_ref, var_ref, m2_unb_ref, b_mean, b_var, rm0, rv0):
        mom, eps = a['momentum'], a['eps']
        self.compare('mean', a['mean'].double(), mean_ref, b_mean)
        inv_ref = 1.0 / (var_ref + eps).sqrt()
        self.compare('invstd', a['invstd'].double(), inv_ref, 0.5 * inv_ref * b_var / (var_ref + eps) + C_BOUND * U24 * inv_ref)
        if rm0 is not None:
            want = (1 - mom) * rm0 + mom * mean_ref
            self.compare('running_mean', a['running_mean'].double(), want, mom * b_mean + C_BOUND * U24 * (want.abs() + rm0.abs()))
        if rv0 is not None:
            want = (1 - mom) * rv0 + mom * m2_unb_ref
            self.compare('running_var', a['running_var'].double(), want, mom * b_var * 2 + C_BOUND * U24 * (want.abs() + rv0.abs()))

    def chk_bn_train_stats(self, a, call):
        x = a['x']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='bn', kind='bn')
        xs = dense64(x).reshape(-1, x.C)
        rm0 = None if a['running_mean'] is None else a['running_mean'].double().clone()
        rv0 = None if a['running_var'] is None else a['running_var'].double().clone()
        out = call()
        P = xs.shape[0]
        m = xs.mean(dim=0)
        d = xs - m
        var = (d * d).mean(dim=0)
        b_mean = sum_bound(m * P, xs, P) / P
        b_var = sum_bound(var * P, d * d, P) / P + 2 * b_mean * d.abs().mean(dim=0)
        self._stats_outputs(a, m, var, var * P / max(P - 1, 1), b_mean, b_var, rm0, rv0)
        return out

    def chk_bn_train_stats_merge(self, a, call):
        C = a['mean'].numel()
        self.meta(geom=(a['slices'], C), family='bn', kind='bn')
        slices = a['slices']
        part = a['partials'][:slices * C * 3].clone()
        rm0 = None if a['running_mean'] is None else a['running_mean'].double().clone()
        rv0 = None if a['running_var'] is None else a['running_var'].double().clone()
        out = call()
        ntot, mean, M2, (n, m, m2) = self._bn_stats_check(None, part, slices, C)
        var = M2 / ntot
        b_mean = sum_bound(mean * ntot, n * m, slices) / ntot
        t = m2 + n * (m - mean) ** 2
        b_var = sum_bound(M2, t, slices) / ntot + 2 * b_mean * (n * (m - mean).abs()).sum(dim=0) / ntot
        self._stats_outputs(a, mean, var, M2 / (ntot - 1).clamp_min(1), b_mean, b_var, rm0, rv0)
        return out

    def chk_bn_train_apply(self, a, call):
        x, y = a['x'], a['y']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='bn', kind='bn')
        xs = dense64(x)
        res = None if a['residual'] is None else dense64(a['residual'])
        snaps = self.snap_out(y)
        amax_before = None if a['amax_out'] is None else a['amax_out'].clone()
        out = call()
        got = dense64(y)
        m, g = a['mean'].double(), a['invstd'].double() * a['gamma'].double()
        b = a['beta'].double()
        pre = (xs - m) * g + b + (0 if res is None else res)
        sl = slope_of(got, a['act'])
        bound = C_BOUND * U24 * ((xs.abs() + m.abs()) * g.abs() + b.abs() + pre.abs() + (0 if res is None else res.abs()) + g.abs() * (xs - m).abs())
        self.compare('bn apply', got, pre * sl, bound * sl.abs())
        self.check_outside(snaps)
        if amax_before is not None:
            self.check_amax_exact(a['amax_out'], amax_before, got)
        return out

    def chk_bn_train_bwd(self, a, call):
        x, y, dy, dx = a['x'], a['y'], a['dy'], a['dx']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='bn', kind='bn')
        xs, ys, dys = dense64(x), dense64(y), dense64(dy)
        snaps = self.snap_out(dx)
        amax_before = None if a['amax_dx'] is None else a['amax_dx'].clone()
        out = call()
        C = x.C
        P = x.N * x.H * x.W
        m, inv, gam = a['mean'].double(), a['invstd'].double(), a['gamma'].double()
        dz = (dys * slope_of(ys, a['act'])).reshape(P, C)
        xh = ((xs.reshape(P, C) - m) * inv)
        sa, sb = dz.sum(dim=0), (dz * xh).sum(dim=0)
        xerr = (xs.reshape(P, C).abs() + m.abs()) * inv
        self.compare('dbeta', a['dbeta'].double(), sa, sum_bound(sa, dz, P))
        self.compare('dgamma', a['dgamma'].double(), sb, sum_bound(sb, dz * xh, P) + C_BOUND * U24 * (dz.abs() * xerr).sum(dim=0))
        # dx from the kernel's OWN sums (checked just above): rounding of the elementwise formula only
        ksa, ksb = a['dbeta'].double(), a['dgamma'].double()
        gi = gam * inv
        ref = gi * (dz - (ksa + xh * ksb) / P)
        bound = C_BOUND * U24 * (gi.abs() * (dz.abs() + (ksa.abs() + xh.abs() * ksb.abs() + xerr * ksb.abs()) / P) + ref.abs())
        got = dense64(dx)
        self.compare('bn dx', got.reshape(P, C), ref, bound)
        self.check_outside(snaps)
        if amax_before is not None:
            self.check_amax_exact(a['amax_dx'], amax_before, got)
        return out

    # ---- elementwise / pooling ------------------------------------------------------------------------------------------
    def chk_act_bwd(self, a, call):
        dy, y, dx = a['dy'], a['y'], a['dx']
        self.meta(geom=(dy.N, dy.H, dy.W, dy.C), family='elementwise', kind='misc')
        dys, ys = dense64(dy), dense64(y)
        snaps = self.snap_out(dx)
        out = call()
        ref = dys * slope_of(ys, a['act'])
        self.compare('act_bwd', dense64(dx), ref, C_BOUND * U24 * ref.abs())
        self.check_outside(snaps)
        return out

    def chk_channel_sum(self, a, call):
        dy, o = a['dy'], a['out']
        self.meta(geom=(dy.N, dy.H, dy.W, dy.C), family='reduction', kind='misc')
        t = dense64(dy).reshape(-1, dy.C)
        out = call()
        ref = t.sum(dim=0)
        self.compare('channel_sum', o.double(), ref, sum_bound(ref, t, t.shape[0]))
        return out

    def chk_add_inplace(self, a, call):
        d, s = a['dst'], a['src']
        self.meta(geom=(d.N, d.H, d.W, d.C), family='elementwise', kind='misc')
        ss = dense64(s)
        snaps = self.snap_out(d)
        out = call()
        ref = self.before_slice(snaps, d) + ss
        self.compare('add_inplace', dense64(d), ref, C_BOUND * U24 * ref.abs())
        self.check_outside(snaps)
        return out

    def chk_zero_insert(self, a, call):
        dy, up, st = a['dy'], a['up'], a['stride']
        self.meta(geom=(dy.N, dy.H, dy.W, dy.C, st), family='copy', kind='misc')
        src = dy.t[..., dy.coff:dy.coff + dy.C].clone()
        snaps = self.snap_out(up)
        out = call()
        ref = torch.zeros((up.N, up.H, up.W, up.C), dtype=torch.float32, device=up.t.device)
        hh, ww = min(dy.H, (up.H + st - 1) // st), min(dy.W, (up.W + st - 1) // st)
        ref[:, 0:hh * st:st, 0:ww * st:st, :] = src[:, :hh, :ww]
        self.exact('zero_insert', up.t[..., up.coff:up.coff + up.C], ref)
        self.check_outside(snaps)
        return out

    def chk_upsample2x(self, a, call):
        x, y = a['x'], a['y']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='copy', kind='misc')
        src = x.t[..., x.coff:x.coff + x.C].clone()
        snaps = self.snap_out(y)
        out = call()
        ref = src.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        self.exact('upsample2x', y.t[..., y.coff:y.coff + y.C], ref)
        self.check_outside(snaps)
        return out

    def chk_upsample2x_bwd(self, a, call):
        dy, dx = a['dy'], a['dx']
        self.meta(geom=(dx.N, dx.H, dx.W, dx.C), family='reduction', kind='misc')
        t = dense64(dy)
        snaps = self.snap_out(dx)
        out = call()
        q = t.view(dx.N, dx.H, 2, dx.W, 2, dx.C)
        ref = q.sum(dim=(2, 4))
        bound = C_BOUND * U24 * q.abs().sum(dim=(2, 4))
        if a['accumulate']:
            b0 = self.before_slice(snaps, dx)
            ref, bound = ref + b0, bound + C_BOUND * U24 * (b0.abs() + ref.abs())
        self.compare('upsample2x_bwd', dense64(dx), ref, bound)
        self.check_outside(snaps)
        return out

    def chk_avgpool2x2(self, a, call):
        x, y = a['x'], a['y']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='reduction', kind='misc')
        t = dense64(x)[:, :x.H // 2 * 2, :x.W // 2 * 2]
        snaps = self.snap_out(y)
        out = call()
        q = t.reshape(x.N, x.H // 2, 2, x.W // 2, 2, x.C)
        ref = q.mean(dim=(2, 4))
        self.compare('avgpool2x2', dense64(y)[:, :x.H // 2, :x.W // 2], ref, C_BOUND * U24 * q.abs().sum(dim=(2, 4)))
        self.check_outside(snaps)
        return out

    def chk_avgpool2x2_bwd(self, a, call):
        dy, dx = a['dy'], a['dx']
        self.meta(geom=(dx.N, dx.H, dx.W, dx.C), family='copy', kind='misc')
        t = dense64(dy)
        snaps = self.snap_out(dx)
        out = call()
        ref = torch.zeros((dx.N, dx.H, dx.W, dx.C), dtype=torch.float64, device=dx.t.device)
        ref[:, :dy.H * 2, :dy.W * 2] = 0.25 * t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        self.compare('avgpool2x2_bwd', dense64(dx), ref, C_BOUND * U24 * ref.abs())
        self.check_outside(snaps)
        return out

    @staticmethod
    def _window_argmax(x, k, stride, pad, Ho, Wo):
        """x: [N, H, W, C] fp32 -> (max [N, Ho, Wo, C], flat input index [N, Ho, Wo, C] of the FIRST maximum in row-major window
        order -- the kernels' tie rule), windows padded with -inf."""
        N, H, W, C = x.shape
        vals, idxs = [], []
        for n in range(N):
            xn = x[n].permute(2, 0, 1).unsqueeze(0)                                     # [1, C, H, W]
            xp = F.pad(xn, (pad, pad, pad, pad), value=-math.inf)
            cols = F.unfold(xp, k, stride=stride).view(C, k * k, Ho * Wo)
            j = torch.argmax(cols, dim=1)                                               # [C, L] (first maximum)
            v = torch.gather(cols, 1, j.unsqueeze(1)).squeeze(1)
            ho = torch.arange(Ho, device=x.device).repeat_interleave(Wo).view(1, -1)
            wo = torch.arange(Wo, device=x.device).repeat(Ho).view(1, -1)
            hh = ho * stride - pad + j // k
            ww = wo * stride - pad + j % k
            vals.append(v.t().reshape(Ho, Wo, C))
            idxs.append((hh * W + ww).t().reshape(Ho, Wo, C))
            del cols
        return torch.stack(vals), torch.stack(idxs)

    @staticmethod
    def _scatter_windows(dy, idx, H, W):
        """dx[n, idx, c] += dy[n, ho, wo, c] in float64, plus sum|dy| for the bound."""
        N, Ho, Wo, C = dy.shape
        dx = torch.zeros((N, H * W, C), dtype=torch.float64, device=dy.device)
        ab = torch.zeros_like(dx)
        ii = idx.reshape(N, Ho * Wo, C)
        dx.scatter_add_(1, ii, dy.reshape(N, Ho * Wo, C))
        ab.scatter_add_(1, ii, dy.abs().reshape(N, Ho * Wo, C))
        return dx.view(N, H, W, C), ab.view(N, H, W, C)

    def chk_maxpool3x3s2(self, a, call):
        x, y = a['x'], a['y']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='pool', kind='misc')
        xs = x.t[..., x.coff:x.coff + x.C].clone()
        snaps = self.snap_out(y)
        out = call()
        Ho, Wo = (x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1
        v, _ = self._window_argmax(xs, 3, 2, 1, Ho, Wo)
        self.exact('maxpool3x3s2', y.t[:, :Ho, :Wo, y.coff:y.coff + y.C], v)
        self.check_outside(snaps)
        return out

    def chk_maxpool3x3s2_bwd(self, a, call):
        x, dy, dx = a['x'], a['dy'], a['dx']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='pool', kind='misc')
        xs = x.t[..., x.coff:x.coff + x.C].clone()
        dys = dense64(dy)
        snaps = self.snap_out(dx)
        out = call()
        _, idx = self._window_argmax(xs, 3, 2, 1, dy.H, dy.W)
        ref, ab = self._scatter_windows(dys, idx, x.H, x.W)
        self.compare('maxpool3x3s2_bwd (first maximum)', dense64(dx), ref, C_BOUND * U24 * ab)
        self.check_outside(snaps)
        return out

    def chk_spp(self, a, call):
        x, outs = a['x'], (a['y5'], a['y9'], a['y13'])
        self.meta(geom=(x.N, x.H, x.W, x.C), family='pool', kind='misc')
        xs = x.t[..., x.coff:x.coff + x.C].clone()
        snaps = self.snap_out(*outs)
        out = call()
        for k, v in zip((5, 9, 13), outs):
            ref, _ = self._window_argmax(xs, k, 1, k // 2, x.H, x.W)
            self.exact('spp %d' % k, v.t[..., v.coff:v.coff + v.C], ref)
        self.check_outside(snaps)
        return out

    def chk_spp_bwd(self, a, call):
        x, dy, dx = a['x'], a['dy'], a['dx']
        C = x.C
        self.meta(geom=(x.N, x.H, x.W, C), family='pool', kind='misc')
        xs = x.t[..., x.coff:x.coff + C].clone()
        dys = dense64(dy)
        snaps = self.snap_out(dx)
        out = call()
        ref, ab = dys[..., :C].clone(), dys[..., :C].abs()
        for j, k in enumerate((5, 9, 13)):
            _, idx = self._window_argmax(xs, k, 1, k // 2, x.H, x.W)
            r, b = self._scatter_windows(dys[..., (j + 1) * C:(j + 2) * C].contiguous(), idx, x.H, x.W)
            ref, ab = ref + r, ab + b
        self.compare('spp_bwd (first maximum)', dense64(dx), ref, C_BOUND * U24 * ab)
        self.check_outside(snaps)
        return out

    def chk_dropblock_apply(self, a, call):
        x, y, m, sc = a['x'], a['y'], a['mask'], a['scale']
        self.meta(geom=(x.N, x.H, x.W, x.C), family='elementwise', kind='misc')
        xs = dense64(x)
        snaps = self.snap_out(y)
        out = call()
        ref = xs * m.double() * sc.double()
        self.compare('dropblock_apply', dense64(y), ref, C_BOUND * U24 * ref.abs())
        self.check_outside(snaps)
        return out

    def chk_dropblock_mask(self, a, call):
        m, sc = a['mask'], a['scale']
        self.meta(geom=tuple(m.shape), family='random', kind='misc')
        out = call()
        if m.is_cuda:
            torch.cuda.synchronize()
        ok = bool(((m == 0) | (m == 1)).all())
        if not ok:
            self.fail('mask values not in {0, 1}')
        ref = torch.tensor([m.numel() / float(m.double().sum())], dtype=torch.float64, device=m.device)
        self.compare('dropblock scale', sc.double(), ref, C_BOUND * U24 * ref.abs())
        return out

    def chk_sgd_momentum(self, a, call):
        p, g, v = a['param'], a['grad'], a['velocity']
        self.meta(geom=(p.numel(),), family='optimizer', kind='misc')
        p0, g0, v0 = p.double().clone(), g.double().clone(), v.double().clone()
        out = call()
        lr, mu, wd = a['lr'], a['momentum'], a['weight_decay']
        d = g0 + wd * p0
        nv = d if a['first_step'] else mu * v0 + d
        bd = C_BOUND * U24 * (g0.abs() + 2 * abs(wd) * p0.abs() + (0 if a['first_step'] else 2 * mu * v0.abs()))
        self.compare('velocity', v.double(), nv, bd)
        ref = p0 - lr * nv
        self.compare('param', p.double(), ref, C_BOUND * U24 * (p0.abs() + 2 * abs(lr) * nv.abs()) + abs(lr) * bd)
        return out

    def chk_ema_update(self, a, call):
        s, p = a['shadow'], a['param']
        self.meta(geom=(s.numel(),), family='optimizer', kind='misc')
        s0, p0 = s.double().clone(), p.double()
        decay = call()
        ref = decay * s0 + (1 - decay) * p0
        self.compare('ema', s.double(), ref, C_BOUND * U24 * (s0.abs() + p0.abs() + ref.abs()))
        return decay

    def chk_yolov3_loss(self, a, call):
        """One head level of YOLOv3Loss: oracle/train_oracle.yolov3_loss in float64 on the launch's own head output (its terms, and
        d(sum of terms)/d(output) by autograd).  Cells whose discrete decisions (ignore mask, IoU threshold) differ between the
        fp32 and the float64 oracle are excluded from the dout comparison and counted; the loss terms are then held to that fp32
        evaluation's own distance as well.  The tracked maximum of dout is exact."""
        import types
        from oracle import train_oracle as tro
        ho, dout = a['head_out'], a['dout']
        an, C = len(a['anchors_px']), a['num_classes']
        self.meta(geom=(ho.N, ho.H, ho.W, ho.C), family='loss', kind='misc')
        cfg = types.SimpleNamespace(
            head=dict(anchors=[list(v) for v in a['anchors_px']], anchor_masks=[list(range(an))], downsample=[a['downsample']],
                      num_classes=C, iou_aware=bool(a['iou_aware'])),
            yolo_loss=dict(scale_x_y=a['scale_x_y'], ignore_thresh=a['ignore_thresh']),
            iou_loss=dict(loss_weight=a['iou_loss_weight'], loss_square=bool(a['iou_loss_square'])),
            iou_aware_loss=dict(loss_weight=a['iou_aware_loss_weight']))
        out_nchw = ho.t[..., ho.coff:ho.coff + ho.C].permute(0, 3, 1, 2).contiguous()
        tgt, gt = a['target'], a['gt_box']
        loss_before = a['loss6'].double().clone()
        amax_before = None if a['amax_dout'] is None else a['amax_dout'].clone()
        snaps = self.snap_out(dout)
        res = call()

        def oracle(dtype):
            o = out_nchw.cpu().to(dtype).requires_grad_(True)            # (the oracle builds its constants on the CPU)
            with torch.enable_grad():
                terms = tro.yolov3_loss([o], [tgt.cpu().to(dtype)], gt.cpu().to(dtype), cfg)
                vals = [terms[k] for k in terms]
                (g,) = torch.autograd.grad(sum(vals), o)
            dev = ho.t.device
            return torch.stack([v.detach().to(torch.float64) for v in vals]).to(dev), g.double().permute(0, 2, 3, 1).to(dev)
        l64, d64 = oracle(torch.float64)
        l32, d32 = oracle(torch.float32)
        # a discrete decision that differs between two evaluations moves a cell's gradient by O(its size); rounding by O(2^-24)
        cell = lambda t: t.reshape(ho.N, ho.H, ho.W, -1)
        scale = d64.abs().amax()
        flip = ((d32 - d64).abs() > 1e-3 * scale).reshape(ho.N, ho.H, ho.W, -1).any(dim=3, keepdim=True).expand_as(cell(d64))
        self.meta(excluded_cells=int(flip[..., 0].sum()))
        got = dense64(dout)
        bound = C_BOUND * (U24 * (d64.abs() + scale) + (d32 - d64).abs())
        self.compare('yolov3_loss dout', torch.where(flip, d64, got), d64, bound)
        n = l64.numel()
        ref = l64 + (loss_before[:n] if a['accumulate'] else 0)
        lb = C_BOUND * (U24 * (ref.abs() + math.sqrt(out_nchw.numel()) * l64.abs()) + (l32 - l64).abs())
        if bool(flip.any()):
            lb = lb + l64.abs() * 1e-3
        self.compare('yolov3_loss terms', a['loss6'].double()[:n], ref, lb)
        if amax_before is not None:
            self.check_amax_exact(a['amax_dout'], amax_before, got)
        self.check_outside(snaps)
        return res

    # ---- reporting ------------------------------------------------------------------------------------------------------
    def summary(self):
        """{(op, family): (launches, worst ratio, median ratio)}."""
        by = collections.defaultdict(list)
        for r in self.census:
            by[(r['op'], r.get('family'))].append(r['ratio'])
        out = {}
        for k, v in sorted(by.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
            v = sorted(v)
            out[k] = (len(v), v[-1], v[len(v) // 2])
        return out

    def report(self, title=''):
        lines = ['launch replay %s: %d checked launches, %d failures, %d declined' % (title, len(self.census), len(self.failures), len(self.declined))]
        for (op, fam), (n, worst, med) in self.summary().items():
            lines.append('  %-26s %-18s n=%4d  worst err/bound %.3f  median %.3f' % (op, fam, n, worst, med))
        if self.unchecked:
            lines.append('  unchecked: %s' % dict(self.unchecked))
        for f in self.failures[:20]:
            lines.append('  FAIL %s' % f)
        return '\n'.join(lines)


def _r32(c):
    return (c + 31) // 32 * 32
