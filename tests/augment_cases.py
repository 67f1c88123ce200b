"""Hand-built recipes for the training-batch kernels (csrc/augment.hip canvas_px / color_px / render_px) at the places the seeded
recipes of g19_augment need not reach -- device-free TEST INFRASTRUCTURE (tests/test_augment_cases.py checks every promise on
the CPU, tests/test_gpu_augment_edges.py runs the kernels against tests/augment_ref.py on the same recipes).

A case is dict(name, family, why, recipe, S, to_rgb, promise): `recipe` has the shape TrainBatchBuilder.plan emits, `S` is the
output size its resize plan was made for, `promise(case)` asserts on the CPU that the case reaches what its name says.  Every
source is at most 24 x 24 and built from patterns (0 / 255 stripes, checkerboards, flat 255, flat 0, grey ramps, primaries)
with a little seeded noise where a flat neighbourhood would hide an index error.

Families: colour (op order and dtype chain), expand (the astype(uint8) wrap and the fill border), mixup (coverage and the
float32 blend), crop (degenerate windows and the flip), render (the resize modes of resize_plan on crops and tiny canvases),
overshoot (8-bit CUBIC / LANCZOS4 accumulators beyond [0, 255]).
"""
import functools
import itertools

import numpy as np

import augment_ref as R
from config import PPYOLO_2x_Config
from ppyolo_hip import augment as A

FILL = np.array([123, 116, 103], np.uint8)
MAX_SIDE = 24
DT = {A.U8: np.uint8, A.F32: np.float32, A.F64: np.float64}
DT_NAME = {A.U8: 'u8', A.F32: 'f32', A.F64: 'f64'}
INTERP_NAME = {A.NEAREST: 'nearest', A.LINEAR: 'linear', A.AREA: 'area', A.CUBIC: 'cubic', A.LANCZOS4: 'lanczos4'}
OP_NAME = {A.OP_BRIGHTNESS: 'b', A.OP_CONTRAST: 'c', A.OP_SATURATION: 's', A.OP_HUE: 'h'}


@functools.lru_cache(maxsize=None)
def builder():
    """The configuration whose mean / std / table the expected images use (no device)."""
    return A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')


# ---------------------------------------------------------------------------------------------------------------------
# sources (uint8 BGR [h, w, 3])

def _src(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3 and a.shape[0] <= MAX_SIDE and a.shape[1] <= MAX_SIDE, a.shape
    return a


def flat(h, w, v):
    return _src(np.full((h, w, 3), v))


def stripes(h, w, pattern=(0, 255), axis=1):
    """0 / 255 stripes: `pattern` repeated along `axis`, all three channels."""
    p = np.resize(np.array(pattern), (w if axis == 1 else h,))
    a = np.broadcast_to(p[None, :] if axis == 1 else p[:, None], (h, w))
    return _src(np.repeat(a[:, :, None], 3, 2))


def checker(h, w):
    yy, xx = np.mgrid[:h, :w]
    return _src(np.repeat((((yy + xx) & 1) * 255)[:, :, None], 3, 2))


def blue_ramp():
    """16 x 16, every value 0 .. 255 once in channel 0 (blue of BGR), the others 0."""
    a = np.zeros((16, 16, 3))
    a[..., 0] = np.arange(256).reshape(16, 16)
    return _src(a)


def palette(h, w, seed):
    """Rows of pure blue / green / red ramps, a grey ramp, flat 0, flat 255, a checkerboard row, then seeded noise."""
    a = np.zeros((h, w, 3))
    ramp = np.linspace(15, 255, w)
    for k in range(min(3, h)):
        a[k, :, k] = ramp
    if h > 3:
        a[3] = ramp[:, None]
    if h > 5:
        a[5] = 255
    if h > 6:
        a[6] = ((np.arange(w) & 1) * 255)[:, None]
    if h > 7:
        a[7:] = np.random.RandomState(seed).randint(0, 256, (h - 7, w, 3))
    return _src(a)


def textured(h, w, seed):
    """A checkerboard of 0 / 255 with seeded noise on every second 2 x 2 block: no two neighbourhoods are alike."""
    a = checker(h, w).astype(np.int64)
    n = np.random.RandomState(seed).randint(0, 256, (h, w, 3))
    yy, xx = np.mgrid[:h, :w]
    m = (((yy >> 1) + (xx >> 1)) & 1).astype(bool)
    a[m] = n[m]
    return _src(a)


def framed(h, w, cy, cx, ch, cw, seed):
    """Seeded noise in the window [cy, cy+ch) x [cx, cx+cw), 0 / 255 stripes of period 2 (vertical and horizontal, xor) around."""
    yy, xx = np.mgrid[:h, :w]
    a = np.repeat(((((yy >> 0) ^ (xx >> 0)) & 1) * 255)[:, :, None], 3, 2).astype(np.int64)
    a[::3] = 255 - a[::3]                                  # (break the checkerboard's symmetry under a flip)
    a[cy:cy + ch, cx:cx + cw] = np.random.RandomState(seed).randint(64, 192, (ch, cw, 3))
    return _src(a)


# ---------------------------------------------------------------------------------------------------------------------
# recipes

def hue(delta):
    return (A.OP_HUE, delta, A._hue_matrix(delta))


def op(code, delta):
    return hue(delta) if code == A.OP_HUE else (code, delta, None)


OPS_OF = {A.U8: [], A.F32: [op(A.OP_CONTRAST, 1.2345), op(A.OP_BRIGHTNESS, 0.75)],
          A.F64: [op(A.OP_SATURATION, 0.8), hue(7.0)]}


def recipe(image, S, interp, ops=(), mix=None, factor=None, expand=None, crop=None, flip=False):
    ops = list(ops)
    color_dtype = A._color_dtype(ops)
    canvas_dtype = A.U8 if expand is not None else color_dtype
    mh, mw = image.shape[:2]
    if mix is not None:
        mh, mw = max(mh, mix.shape[0]), max(mw, mix.shape[1])
    H, W = expand[:2] if expand is not None else (mh, mw)
    crop = tuple(crop) if crop is not None else (0, 0, H, W)
    ch, cw = crop[2], crop[3]
    fx, fy = float(S) / cw, float(S) / ch
    return dict(image=image, mix_image=mix, factor=factor, ops=ops, color_dtype=color_dtype, expand=expand, fill=FILL,
                crop=crop, flip=bool(flip), canvas_dtype=canvas_dtype, interp=int(interp), fx=fx, fy=fy,
                resize=A.resize_plan(ch, cw, fx, fy, int(interp), canvas_dtype))


CASES = {}


def add(name, family, why, rec, S, promise, to_rgb=True, **extra):
    assert name not in CASES, name
    CASES[name] = dict(name=name, family=family, why=why, recipe=rec, S=S, to_rgb=to_rgb, promise=promise, **extra)


def family(fam):
    return [c for c in CASES.values() if c['family'] == fam]


@functools.lru_cache(maxsize=None)
def expected_canvas(name):
    """augment_ref.canvas of the case (shared: do not modify)."""
    c = CASES[name]
    out = R.canvas(c['recipe'], c['to_rgb'])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_image(name):
    """augment_ref.images of the case alone -> float32 [3, S, S] (shared: do not modify)."""
    c, b = CASES[name], builder()
    out = R.images([c['recipe']], b.mean, b.std, c['to_rgb'])[0]
    out.setflags(write=False)
    return out


def stage(rec, to_rgb=True):
    """The colour-stage image of a recipe: augment_ref.canvas without expand / crop / flip (the values BEFORE the expand cast)."""
    mh, mw = rec['image'].shape[:2]
    if rec['mix_image'] is not None:
        mh, mw = max(mh, rec['mix_image'].shape[0]), max(mw, rec['mix_image'].shape[1])
    return R.canvas(dict(rec, expand=None, crop=(0, 0, mh, mw), flip=False), to_rgb)


# ---------------------------------------------------------------------------------------------------------------------
# colour order

CD = builder().cd
_ENDS = {A.OP_BRIGHTNESS: CD['brightness'][:2], A.OP_CONTRAST: CD['contrast'][:2], A.OP_SATURATION: CD['saturation'][:2],
         A.OP_HUE: CD['hue'][:2]}
# hue's ends +-18 are whole turns of delta * pi: its two further deltas keep the rotation visible
_HUE_INNER = (-17.75, 17.5)


def _ops_at_ends(order, k):
    """Deltas at the ends of the ranges TrainBatchBuilder._color draws from, the end alternating with the op's place and k."""
    out = []
    for j, code in enumerate(order):
        lo_hi = _ENDS[code]
        d = lo_hi[(j + k) & 1]
        if code == A.OP_HUE and (k >> 1) & 1:
            d = _HUE_INNER[(j + k) & 1]
        out.append(op(code, float(d)))
    return out


def _promise_colour(c):
    r = c['recipe']
    codes = [o[0] for o in r['ops']]
    want = A.U8 if not codes else (A.F64 if codes[-1] == A.OP_HUE else A.F32)
    assert r['color_dtype'] == r['canvas_dtype'] == want == c['dtype']
    cv = expected_canvas(c['name'])
    assert cv.dtype == DT[want] and cv.shape == r['image'].shape
    if len(codes) >= 2 and A.OP_BRIGHTNESS in codes:
        # brightness adds, the other three scale: reversing the order moves the addition across a scaling, so the image changes
        other = R.canvas(dict(r, ops=r['ops'][::-1]))
        assert other.shape == cv.shape and not np.array_equal(other.astype(np.float64), cv.astype(np.float64))


_PAL = palette(8, 12, 1)
for _k, _order in enumerate(itertools.permutations([A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE])):
    _ops = _ops_at_ends(_order, _k)
    add('colour_' + ''.join(OP_NAME[o] for o in _order), 'colour',
        'op order %s with deltas at the ends of their ranges' % '>'.join(OP_NAME[o] for o in _order),
        recipe(_PAL, 8, A.NEAREST, _ops), 8, _promise_colour, dtype=A._color_dtype(_ops))
for _order in ((A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE), (A.OP_HUE, A.OP_SATURATION, A.OP_CONTRAST, A.OP_BRIGHTNESS)):
    for _n in range(0 if _order[0] == A.OP_BRIGHTNESS else 1, 4):
        _ops = _ops_at_ends(_order[:_n], 1)
        _nm = 'colour_prefix%d_%s' % (_n, ''.join(OP_NAME[o] for o in _order[:_n]) or 'none')
        add(_nm, 'colour', 'the first %d ops of %s: %s' % (_n, ''.join(OP_NAME[o] for o in _order), DT_NAME[A._color_dtype(_ops)]),
            recipe(_PAL, 8, A.NEAREST, _ops), 8, _promise_colour, dtype=A._color_dtype(_ops))


# ---------------------------------------------------------------------------------------------------------------------
# expand wrap

WRAP_CLASSES = ['below 0 with a fraction', 'below 0 and integral', 'in (255, 256)', 'in [256, 512)', '>= 512']


def wrap_classes(v):
    """-> the number of values of v in each of WRAP_CLASSES."""
    v = np.asarray(v, np.float64).ravel()
    t = np.trunc(v)
    return [int(((v < 0) & (v != t)).sum()), int(((v < 0) & (v == t)).sum()), int(((v > 255) & (v < 256)).sum()),
            int(((v >= 256) & (v < 512)).sum()), int((v >= 512).sum())]


# No matrix of _hue_matrix gives an exactly integral negative float64 (its entries are sums of products of three-digit decimals):
# this one is dyadic, so products and sums are exact and every class of the float64 stage exists.  Rows are input channels.
DYADIC_T = np.array([[1.0, -0.5, 2.5], [-0.25, 1.0, 0.0], [0.0, -1.0, 1.0078125]])

_BLUE = blue_ramp()
_PAL16 = palette(16, 16, 2)
STAGES = [
    ('f32_sat_bri', _BLUE, [op(A.OP_SATURATION, 1.5), op(A.OP_BRIGHTNESS, 1.25)]),
    ('f32_con_sat', _PAL16, [op(A.OP_CONTRAST, 1.5), op(A.OP_SATURATION, 1.5)]),
    ('f64_con_sat_hue', _PAL16, [op(A.OP_CONTRAST, 1.5), op(A.OP_SATURATION, 1.5), hue(7.3)]),
    ('f64_bri_hue', _BLUE, [op(A.OP_BRIGHTNESS, 0.6), hue(-18.0)]),
    ('f64_dyadic', _PAL16, [op(A.OP_CONTRAST, 1.5), (A.OP_HUE, 0.0, DYADIC_T)]),
]
# (name, expand (eh, ew, ey, ex), crop or None, flip, pixels of the crop inside the image: 'all' / 'none' / 'some')
PLACEMENTS = [
    ('top_left', (22, 20, 0, 0), None, False, 'some'),
    ('top_right', (22, 20, 0, 4), None, False, 'some'),
    ('bottom_left', (22, 20, 6, 0), None, False, 'some'),          # ey + mh == eh
    ('bottom_right', (22, 20, 6, 4), None, True, 'some'),
    ('same_size', (16, 16, 0, 0), None, False, 'all'),
    ('crop_in_fill', (24, 24, 8, 8), (1, 0, 6, 7), False, 'none'),
    ('straddle_left', (24, 24, 4, 4), (6, 1, 5, 6), False, 'some'),
    ('straddle_right', (24, 24, 4, 4), (6, 17, 5, 6), True, 'some'),
    ('straddle_top', (24, 24, 4, 4), (1, 6, 6, 5), True, 'some'),
    ('straddle_bottom', (24, 24, 4, 4), (17, 6, 6, 5), False, 'some'),
    ('crop_in_image', (24, 24, 4, 4), (5, 6, 14, 13), False, 'all'),
]


def _promise_expand(c):
    r = c['recipe']
    eh, ew, ey, ex = r['expand']
    cy, cx, ch, cw = r['crop']
    mh, mw = r['image'].shape[:2]
    assert r['canvas_dtype'] == A.U8 and r['color_dtype'] == c['dtype'] != A.U8
    yy, xx = np.mgrid[cy:cy + ch, cx:cx + cw]
    inside = (yy >= ey) & (yy < ey + mh) & (xx >= ex) & (xx < ex + mw)
    assert {'all': inside.all(), 'none': not inside.any(), 'some': inside.any() and not inside.all()}[c['inside']]
    cv = expected_canvas(c['name'])
    if r['flip']:
        inside = inside[:, ::-1]
    assert cv.dtype == np.uint8 and (cv[~inside] == FILL).all()
    if inside.any():                                    # the wrapped values are not the fill: a shifted border would show
        assert (cv[inside] != FILL).any(axis=-1).mean() > 0.9
    st = stage(r)
    assert st.dtype == DT[c['dtype']]
    got = wrap_classes(st)
    assert all(g > 0 for g, need in zip(got, c['classes']) if need), (c['name'], got)


_STAGE_CLASSES = {'f32_sat_bri': [1, 1, 1, 1, 0], 'f32_con_sat': [1, 0, 0, 1, 1], 'f64_con_sat_hue': [1, 0, 0, 1, 1],
                  'f64_bri_hue': [0, 0, 1, 0, 0], 'f64_dyadic': [1, 1, 0, 1, 1]}
for _i, (_pn, _ex, _crop, _flip, _inside) in enumerate(PLACEMENTS):
    for _j, (_sn, _img, _ops) in enumerate(STAGES):
        if _pn not in ('top_left', 'crop_in_image') and (_i + _j) % len(STAGES) > 1:
            continue                                    # every stage at two placements in full, two stages at each other placement
        add('expand_%s_%s' % (_pn, _sn), 'expand',
            'colour stage %s wrapped by astype(uint8) into an expand canvas, placement %s' % (_sn, _pn),
            recipe(_img, 8, A.NEAREST, _ops, expand=_ex, crop=_crop, flip=_flip), 8, _promise_expand,
            dtype=A._color_dtype(_ops), inside=_inside, classes=_STAGE_CLASSES[_sn], stage=_sn, placement=_pn)


# ---------------------------------------------------------------------------------------------------------------------
# mixup

# F_254: found by scanning k / 1000 on the CPU -- the flat-255 blend f32(255 * f32(f)) + f32(255 * f32(1 - f)) is 254.99998 there
# and astype(uint8) truncates it to 254 (0.001, 0.5 and 0.999 give 255).  F_NOT_ONE: the two float32 weights f32(f) and f32(1 - f)
# do not sum to 1 (taken exactly; rounded to float32 their sum is 1 for every f, the error never exceeds half an ulp of 1).
F_254 = 0.008
F_NOT_ONE = 1.0 / 3.0
MIX_FACTORS = [1e-3, 0.5, 0.999, F_NOT_ONE, F_254]


def _promise_mixup(c):
    r = c['recipe']
    (h0, w0), (h1, w1) = r['image'].shape[:2], r['mix_image'].shape[:2]
    cv = expected_canvas(c['name'])
    assert r['factor'] == c['factor'] and 0.0 < r['factor'] < 1.0
    if c['coverage']:
        mh, mw = max(h0, h1), max(w0, w1)
        yy, xx = np.mgrid[:mh, :mw]
        in0, in1 = (yy < h0) & (xx < w0), (yy < h1) & (xx < w1)
        for m in (in0 & in1, in0 & ~in1, ~in0 & in1, ~in0 & ~in1):
            assert m.any()
        if not r['ops'] and r['expand'] is None:
            assert cv.shape == (mh, mw, 3) and not cv[~in0 & ~in1].any()        # covered by neither image: zeros
            if 0.25 <= r['factor'] <= 0.75:                                      # (at 0.001 / 0.999 one image alone rounds to 0)
                assert cv[in0 & in1].any() and cv[in0 & ~in1].any() and cv[~in0 & in1].any()
    if c['to_rgb'] is False:
        assert not np.array_equal(cv, R.canvas(r, True))                         # the channel order shows


def _promise_mixup_flat(c):
    r = c['recipe']
    cv = expected_canvas(c['name'])
    assert (r['image'] == 255).all() and (r['mix_image'] == 255).all() and cv.dtype == np.uint8
    assert len(np.unique(cv)) == 1 and int(cv[0, 0, 0]) in (254, 255)
    if c['factor'] == F_254:
        assert (cv == 254).all()


_MA, _MB = textured(5, 12, 3), palette(7, 9, 4)
for _f in MIX_FACTORS:
    for _rgb in (True, False):
        add('mixup_5x12_7x9_f%r_%s' % (_f, 'rgb' if _rgb else 'bgr'), 'mixup',
            '5 x 12 blended with 7 x 9 at factor %r: both, only one, neither' % _f,
            recipe(_MA, 8, A.NEAREST, mix=_MB, factor=_f), 8, _promise_mixup, to_rgb=_rgb, factor=_f, coverage=True)
    add('mixup_flat255_f%r' % _f, 'mixup', 'both images flat 255 at factor %r: the float32 blend is 255 or 254.99998 (-> 254)' % _f,
        recipe(flat(6, 6, 255), 8, A.NEAREST, mix=flat(6, 6, 255), factor=_f), 8, _promise_mixup_flat, factor=_f, coverage=False)
add('mixup_then_colour_f32', 'mixup', 'the truncated blend feeds contrast > brightness (float32 canvas), first image the larger one',
    recipe(_MB, 8, A.NEAREST, OPS_OF[A.F32], mix=np.ascontiguousarray(_MA[:4, :6]), factor=0.5), 8, _promise_mixup, factor=0.5, coverage=False)
add('mixup_then_hue_expand_crop_flip', 'mixup', 'mixup > saturation > hue > expand > crop over the neither-covered corner > flip',
    recipe(_MA, 8, A.NEAREST, OPS_OF[A.F64], mix=_MB, factor=F_NOT_ONE, expand=(11, 15, 2, 2), crop=(5, 8, 6, 7), flip=True), 8,
    _promise_mixup, to_rgb=False, factor=F_NOT_ONE, coverage=True)


# ---------------------------------------------------------------------------------------------------------------------
# crop / flip

def _promise_crop(c):
    r = c['recipe']
    H, W = r['image'].shape[:2]
    cy, cx, ch, cw = r['crop']
    assert (ch, cw) == c['window'] and cy + ch <= H and cx + cw <= W
    if c['last_row']:
        assert cy + ch == H
    if c['last_col']:
        assert cx + cw == W
    cv = expected_canvas(c['name'])
    assert cv.shape == (ch, cw, 3) and cv.dtype == DT[r['canvas_dtype']]
    other = R.canvas(dict(r, flip=not r['flip']))
    assert np.array_equal(other[:, ::-1], cv)
    assert (cw == 1) == np.array_equal(other, cv)                   # the flip shows wherever there is more than one column


_CROP_SRC = {9: textured(8, 9, 5), 10: textured(9, 10, 6)}         # odd and even widths
for _w, _img in _CROP_SRC.items():
    _h = _img.shape[0]
    for _wn, (_cy, _cx, _ch, _cw) in (('1x1', (3, 4, 1, 1)), ('1x1_last', (_h - 1, _w - 1, 1, 1)), ('1xN', (2, 1, 1, _w - 2)),
                                       ('1xN_last_row', (_h - 1, 0, 1, _w)), ('Nx1', (1, 3, _h - 2, 1)),
                                       ('Nx1_last_col', (0, _w - 1, _h, 1)), ('odd_last', (_h - 3, _w - 5, 3, 5)),
                                       ('even_last', (_h - 4, _w - 4, 4, 4)), ('full', (0, 0, _h, _w))):
        for _flip in (False, True):
            _dt = (A.U8, A.F32, A.F64)[(_cy + _cx + _flip) % 3]
            add('crop_w%d_%s_%s%s' % (_w, _wn, DT_NAME[_dt], '_flip' if _flip else ''), 'crop',
                'window %s of a %d-wide canvas%s, upscaled bilinearly' % (_wn, _w, ', flipped' if _flip else ''),
                recipe(_img, 8, A.LINEAR, OPS_OF[_dt], crop=(_cy, _cx, _ch, _cw), flip=_flip), 8, _promise_crop,
                window=(_ch, _cw), last_row=_cy + _ch == _h, last_col=_cx + _cw == _w)


# ---------------------------------------------------------------------------------------------------------------------
# render geometry

def taps(p):
    """The unclamped range of the taps that count (non-zero weight) of a plan: (x lowest, x highest, y lowest, y highest)."""
    def axis(first, w, k):
        if p['mode'] != A.MODE_SEP:
            return int(first.min()), int(first.max()) + (1 if p['mode'] == A.MODE_NEAREST else k) - 1
        idx = (first[:, None] + np.arange(w.shape[1])[None, :])[w != 0]
        return int(idx.min()), int(idx.max())
    return axis(p['xfirst'], p['xw'], p['ix']) + axis(p['yfirst'], p['yw'], p['iy'])


def canvas_clamped_image(rec, to_rgb=True, pad=8):
    """The WRONG resize the crop cases must tell from the right one: taps beyond the crop window read the canvas around it
    (clamped to the canvas, not to the crop) -> resized [S, S, 3] in the canvas dtype."""
    H, W = rec['expand'][:2] if rec['expand'] is not None else stage(rec, to_rgb).shape[:2]
    full = R.canvas(dict(rec, crop=(0, 0, H, W), flip=False), to_rgb)
    cy, cx, ch, cw = rec['crop']
    x = np.arange(-pad, cw + pad)
    X = np.clip((cw - 1 - x if rec['flip'] else x) + cx, 0, W - 1)
    Y = np.clip(np.arange(-pad, ch + pad) + cy, 0, H - 1)
    p = dict(rec['resize'])
    kx, ky = p['xw'].shape[1] + p['ix'], p['yw'].shape[1] + p['iy']
    assert p['xfirst'].min() >= -pad and p['xfirst'].max() + kx <= cw + pad
    assert p['yfirst'].min() >= -pad and p['yfirst'].max() + ky <= ch + pad
    p['xfirst'], p['yfirst'] = p['xfirst'] + pad, p['yfirst'] + pad
    return R.resize(np.ascontiguousarray(full[Y][:, X]), dict(resize=p))


def plan_facts(p):
    """What a plan is, in the words the case names use."""
    sep = p['mode'] == A.MODE_SEP
    return dict(mode=p['mode'], fixpt=p['fixpt'], ix=p['ix'], iy=p['iy'], kx=p['xw'].shape[1] if sep else 1,
                ky=p['yw'].shape[1] if sep else 1)


def _promise_render(c):
    r = c['recipe']
    p = r['resize']
    assert (p['dw'], p['dh']) == (c['S'], c['S']) and r['canvas_dtype'] == c['dtype']
    facts = plan_facts(p)
    for k, v in c['expect'].items():
        if callable(v):
            assert v(facts[k]), (c['name'], k, facts[k])
        else:
            assert facts[k] == v, (c['name'], k, facts[k], v)
    assert expected_image(c['name']).shape == (3, c['S'], c['S'])
    if c.get('rows_vary'):                              # _area_table: the number of non-zero taps differs from row to row
        assert len(set((p['xw'] != 0).sum(1))) > 1 or len(set((p['yw'] != 0).sum(1))) > 1
    if c.get('inside_crop'):
        cy, cx, ch, cw = r['crop']
        H, W = r['image'].shape[:2]
        assert 0 < cy and cy + ch < H and 0 < cx and cx + cw < W
        lo_x, hi_x, lo_y, hi_y = taps(p)
        leaves = lo_x < 0 or hi_x > cw - 1 or lo_y < 0 or hi_y > ch - 1
        assert leaves == c['leaves'], (c['name'], lo_x, hi_x, lo_y, hi_y)
        right = R.resize(np.array(expected_canvas(c['name'])), r)
        wrong = canvas_clamped_image(r)
        # taps that stay inside the window cannot read across its border; those that leave it must be clamped to it
        assert np.array_equal(right, wrong) == (not leaves), c['name']


def _expect_generic(interp, dt, **over):
    k = {A.LINEAR: 2, A.AREA: 2, A.CUBIC: 4, A.LANCZOS4: 8}.get(interp, 1)
    e = dict(mode=A.MODE_NEAREST if interp == A.NEAREST else A.MODE_SEP, fixpt=int(dt == A.U8 and interp != A.NEAREST), ix=0, iy=0,
             kx=k, ky=k)
    e.update(over)
    return e


def add_render(name, why, img, S, interp, dt, expect, crop=None, flip=False, family_='render', **extra):
    add('%s_%s_%s_%s_S%d' % (family_, name, INTERP_NAME[interp], DT_NAME[dt], S), family_, why,
        recipe(img, S, interp, OPS_OF[dt], crop=crop, flip=flip), S, _promise_render, dtype=dt, expect=expect, **extra)


RENDER_SIZES = [40, 72, 38, 70]         # S % 64 != 0 below and above one 64-wide block; 38 and 70 are no multiple of the 4-row block
_BASE = textured(13, 17, 7)
_FRAMED = framed(20, 22, 6, 7, 9, 8, 8)
_ALL = [A.NEAREST, A.LINEAR, A.AREA, A.CUBIC, A.LANCZOS4]
_DTS = [A.U8, A.F32, A.F64]
for _interp in _ALL:
    for _dt in _DTS:
        for _S in RENDER_SIZES:
            add_render('up_13x17', '13 x 17 upscaled to %d: partial 64 x 4 blocks at the right and bottom edges' % _S, _BASE, _S,
                       _interp, _dt, _expect_generic(_interp, _dt), flip=_dt == A.F32)
        for _flip in (False, True):
            add_render('window%s' % ('_flip' if _flip else ''),
                       'a 9 x 8 window strictly inside a 20 x 22 canvas whose surroundings are 0 / 255 stripes', _FRAMED, 40, _interp,
                       _dt, _expect_generic(_interp, _dt), crop=(6, 7, 9, 8), flip=_flip, inside_crop=True,
                       leaves=_interp in (A.CUBIC, A.LANCZOS4))
        for _nm, _img in (('1x1', textured(3, 3, 9)[1:2, 2:3]), ('1x5', textured(2, 5, 10)[:1]), ('5x1', textured(5, 2, 11)[:, :1]),
                          ('2x2', textured(2, 2, 12))):
            add_render('from_' + _nm, 'upscale of a %s canvas: every tap but one is clamped' % _nm, np.ascontiguousarray(_img), 40,
                       _interp, _dt, _expect_generic(_interp, _dt))

_SQ24, _R23x21 = textured(24, 24, 13), textured(21, 23, 14)
_W24H17, _W24H16, _W24H5 = textured(17, 24, 15), textured(16, 24, 16), textured(5, 24, 17)
_many = lambda k: k >= 3
for _dt in _DTS:
    add_render('down_23x21', 'non-integer AREA downscale: computeResizeAreaTab rows of two to four taps', _R23x21, 10, A.AREA, _dt,
               dict(mode=A.MODE_SEP, fixpt=0, ix=0, iy=0, kx=_many, ky=_many), rows_vary=True)
    add_render('exact2x', 'AREA at exactly 2x: the 2 x 2 block sum, (s + 2) >> 2 for uint8', _SQ24, 12, A.AREA, _dt,
               dict(mode=A.MODE_AREA_FAST, fixpt=0, ix=2, iy=2))
    add_render('exact2x', 'LINEAR at exactly 2x is replaced by AREA', _SQ24, 12, A.LINEAR, _dt,
               dict(mode=A.MODE_AREA_FAST, fixpt=0, ix=2, iy=2))
    add_render('exact2x', 'CUBIC at exactly 2x stays the generic 4-tap path', _SQ24, 12, A.CUBIC, _dt, _expect_generic(A.CUBIC, _dt))
    add_render('exact3x', 'AREA at exactly 3x: rint(s * 1/9) for uint8', _SQ24, 8, A.AREA, _dt,
               dict(mode=A.MODE_AREA_FAST, fixpt=0, ix=3, iy=3))
    add_render('exact3x2', 'AREA at 3x by 2x: a 3 x 2 block, rint(s * 1/6) for uint8', _W24H16, 8, A.AREA, _dt,
               dict(mode=A.MODE_AREA_FAST, fixpt=0, ix=3, iy=2))
    add_render('exact3x', 'LINEAR at exactly 3x is NOT replaced', _SQ24, 8, A.LINEAR, _dt, _expect_generic(A.LINEAR, _dt))
    for _interp in _ALL:
        add_render('identity', 'dsize == ssize: a copy whatever the interpolation', _SQ24, 24, _interp, _dt,
                   dict(mode=A.MODE_NEAREST, fixpt=0, ix=0, iy=0))
    add_render('one_axis_2x', 'x at exactly 2x, y at 17/12: LINEAR stays bilinear', _W24H17, 12, A.LINEAR, _dt,
               _expect_generic(A.LINEAR, _dt))
    add_render('one_axis_2x', 'x at exactly 2x, y at 17/12: AREA takes the table path on both axes, two taps along x', _W24H17, 12,
               A.AREA, _dt, dict(mode=A.MODE_SEP, fixpt=0, ix=0, iy=0, kx=2, ky=_many), rows_vary=True)
    add_render('down_x_up_y', 'x shrinks 2x, y grows 12/5: AREA is the bilinear emulation on both axes', _W24H5, 12, A.AREA, _dt,
               _expect_generic(A.AREA, _dt))


# ---------------------------------------------------------------------------------------------------------------------
# 8-bit overshoot

def fixpt_accumulators(img, p):
    """The 11-bit fixed-point resize of augment_ref.resize with every intermediate kept: (horizontal sums, products hs * wy,
    running vertical sums, final accumulator) as int64 arrays."""
    h, w = img.shape[:2]
    src = img.astype(np.int64)
    kx, ky = p['xw'].shape[1], p['yw'].shape[1]
    xi = lambda k: np.clip(p['xfirst'] + k, 0, w - 1)
    yi = lambda k: np.clip(p['yfirst'] + k, 0, h - 1)
    run, hor_run = 0, []
    for j in range(kx):
        run = run + src[:, xi(j)] * p['xw'][:, j].astype(np.int64)[None, :, None]
        hor_run.append(run)
    hor = run
    prods = [hor[yi(k)] * p['yw'][:, k].astype(np.int64)[:, None, None] for k in range(ky)]
    partial = np.cumsum(np.stack(prods), axis=0)
    return np.stack(hor_run), np.stack(prods), partial, partial[-1]


def _promise_overshoot(c):
    r = c['recipe']
    p = r['resize']
    assert p['mode'] == A.MODE_SEP and p['fixpt'] == 1 and r['canvas_dtype'] == A.U8
    cv = np.array(expected_canvas(c['name']))
    assert set(np.unique(cv)) <= {0, 255}
    hor, prods, partial, acc = fixpt_accumulators(cv, p)
    out = (acc + (1 << 21)) >> 22
    assert np.array_equal(np.clip(out, 0, 255).astype(np.uint8), R.resize(cv, r))
    if c['both_signs']:
        assert out.min() < 0 and out.max() > 255, (out.min(), out.max())
    else:
        assert out.max() > c['beyond'], out.max()
    # the kernel's accumulators are int: every horizontal sum, product and running vertical sum must fit
    worst = max(int(np.abs(a).max()) for a in (hor, prods, partial, acc + (1 << 21)))
    assert worst < 2 ** 31, (c['name'], worst)
    c['worst_accumulator'] = worst


_SIGN = {A.CUBIC: (0, 255, 255, 0), A.LANCZOS4: (0, 255, 0, 255, 255, 0, 255, 0)}
for _interp in (A.CUBIC, A.LANCZOS4):
    _v = stripes(24, 24, _SIGN[_interp], axis=1)
    _prod = np.minimum(_v, stripes(24, 24, _SIGN[_interp], axis=0))
    for _S in (40, 38):
        add('overshoot_stripes_%s_S%d' % (INTERP_NAME[_interp], _S), 'overshoot',
            '0 / 255 columns in the sign pattern of the weights at a half-pixel phase: below 0 between the dark pair, above 255 '
            'between the bright pair', recipe(_v, _S, _interp), _S, _promise_overshoot, both_signs=True, dtype=A.U8)
        add('overshoot_product_%s_S%d' % (INTERP_NAME[_interp], _S), 'overshoot',
            'the same pattern on both axes: the largest accumulator the 8-bit path can reach',
            recipe(_prod, _S, _interp), _S, _promise_overshoot, both_signs=False, beyond=300, dtype=A.U8)


# The worst case of the 8-bit path.  At exactly 2x the generic path samples at 2d + 0.5: every output sits at the half-pixel
# phase, where the positive weights sum to 1.357 and the negative ones to -0.357 (LANCZOS4).  Rows that meet a positive
# vertical weight carry the columns' sign pattern, rows that meet a negative one its inverse, so every product of the vertical
# pass has the same sign: 255 * (2780^2 + 732^2) = 0.981 of 2^31 with the table's integer weights.  No 0 .. 255 input gets higher.
for _interp in (A.CUBIC, A.LANCZOS4):
    _q = np.roll(np.resize(np.array(_SIGN[_interp]), (24,)), 1) > 0
    _xnor = _src(np.repeat(((_q[:, None] == _q[None, :]) * 255)[:, :, None], 3, 2))
    add('overshoot_half_phase_%s_S12' % INTERP_NAME[_interp], 'overshoot',
        'exactly 2x, every output at the half-pixel phase, rows and columns in the sign pattern of the weights and its inverse: the '
        'largest accumulator any uint8 image can produce', recipe(_xnor, 12, _interp), 12, _promise_overshoot, both_signs=False,
        beyond={A.CUBIC: 330, A.LANCZOS4: 480}[_interp], dtype=A.U8)


# ---------------------------------------------------------------------------------------------------------------------
# what csrc/augment.hip's desc_ok states, on the recipe (a descriptor that fails it is skipped silently by the kernels)

def desc_ok(r, S):
    h0, w0 = r['image'].shape[:2]
    h1, w1 = r['mix_image'].shape[:2] if r['mix_image'] is not None else (0, 0)
    mh, mw = max(h0, h1), max(w0, w1)
    cy, cx, ch, cw = r['crop']
    p = r['resize']
    ok = h0 > 0 and w0 > 0 and 0 <= len(r['ops']) <= 4 and ch > 0 and cw > 0
    H, W = r['expand'][:2] if r['expand'] is not None else (mh, mw)
    if r['expand'] is not None:
        ok = ok and H > 0 and W > 0
    ok = ok and cy >= 0 and cx >= 0 and cy + ch <= H and cx + cw <= W
    kx, ky = p['xw'].shape[1], p['yw'].shape[1]
    ok = ok and 0 < kx <= 64 and 0 < ky <= 64
    ok = ok and p['xfirst'].shape == (S,) and p['yfirst'].shape == (S,) and p['xw'].shape == (S, kx) and p['yw'].shape == (S, ky)
    if p['mode'] == A.MODE_AREA_FAST:
        ok = ok and p['ix'] > 0 and p['iy'] > 0 and p['ix'] * S <= cw and p['iy'] * S <= ch
    return bool(ok)


def batches():
    """The cases grouped into launches: {(S, to_rgb): [names]} (one render launch has one S and one channel order)."""
    out = {}
    for c in CASES.values():
        out.setdefault((c['S'], c['to_rgb']), []).append(c['name'])
    return out
