"""The hand recipes of tests/augment_cases.py keep their promises (CPU), and the coefficient tables of augment.resize_plan --
product code that both the device kernel and tests/augment_ref.py apply -- agree with the published definitions of the five
interpolations, evaluated here afresh in float64 without resize_plan or any of its helpers.

RESIZE_BOUND.  The planner rounds sample positions and weights to float32 as OpenCV does; the definition below does not.  The
largest difference over the float64 render cases, measured on the CPU (profiles/augment_resize_definition.txt), in units of
the canvas's value range max|canvas| (positions reach 24, where a float32 is 1e-6 off; one pixel of slope turns that into 1e-6):

    nearest 0    linear 7.16e-07    area 3.70e-08    cubic 1.46e-06    lanczos4 8.07e-07

The bound asserted is four times the measured value per interpolation (a handful of small cases underestimates the tail).  The
self-check perturbs one weight by 2^-10 or shifts one first-tap index by one on a copy of the plan: the same comparison must
then fail, for every interpolation."""
import copy

import numpy as np
import pytest

import augment_cases as C
import augment_ref as R
from ppyolo_hip import augment as A

FAMILIES = ['colour', 'expand', 'mixup', 'crop', 'render', 'overshoot']


# ---------------------------------------------------------------------------------------------------------------------
# 1. the cases

def test_names_families_and_sources():
    assert sorted({c['family'] for c in C.CASES.values()}) == sorted(FAMILIES)
    assert all(name == c['name'] for name, c in C.CASES.items()) and len({c['name'] for c in C.CASES.values()}) == len(C.CASES)
    for c in C.CASES.values():
        assert isinstance(c['why'], str) and len(c['why']) > 10 and callable(c['promise'])
        for im in (c['recipe']['image'], c['recipe']['mix_image']):
            if im is not None:
                assert im.dtype == np.uint8 and im.ndim == 3 and max(im.shape[:2]) <= C.MAX_SIDE, c['name']
    counts = {f: len(C.family(f)) for f in FAMILIES}
    print('AUGMENT-CASES per family:', counts)
    assert all(n >= 8 for n in counts.values())


@pytest.mark.parametrize('fam', FAMILIES)
def test_every_promise_holds(fam):
    for c in C.family(fam):
        c['promise'](c)


@pytest.mark.parametrize('fam', FAMILIES)
def test_every_recipe_packs_and_passes_the_descriptor_checks(fam):
    for c in C.family(fam):
        r, S = c['recipe'], c['S']
        assert C.desc_ok(r, S), c['name']
        blob, lay = A.pack_batch([r], c['to_rgb'], np.zeros(0, np.int64), np.zeros(0, np.float32), None, None, None)
        assert lay['desc'] == 0 and lay['sources'] == [] and blob.dtype == np.uint8 and blob.size >= A.DESC_BYTES
        i64 = blob[:64].view(np.int64)
        p = r['resize']
        n_src = r['image'].size + (r['mix_image'].size if r['mix_image'] is not None else 0)
        assert 0 < i64[0] and i64[0] + r['image'].size <= blob.size and n_src < blob.size         # the sources lie in the blob
        for off, n in ((i64[2], 4 * S), (i64[3], 4 * S * p['xw'].shape[1]), (i64[4], 4 * S), (i64[5], 4 * S * p['yw'].shape[1])):
            assert off % 16 == 0 and 0 < off and off + n <= blob.size, c['name']
    # and a descriptor the kernels would skip is told from these
    bad = dict(C.family(fam)[0]['recipe'], crop=(0, 0, 99, 99))
    assert not C.desc_ok(bad, C.family(fam)[0]['S'])


def test_colour_orders_cover_every_order_prefix_and_dtype():
    cs = C.family('colour')
    orders = {tuple(o[0] for o in c['recipe']['ops']) for c in cs}
    assert len([o for o in orders if len(o) == 4]) == 24
    assert {len(o) for o in orders} == {0, 1, 2, 3, 4}
    assert {c['recipe']['canvas_dtype'] for c in cs} == {A.U8, A.F32, A.F64}
    short = [c for c in cs if 0 < len(c['recipe']['ops']) < 4]
    assert {c['recipe']['color_dtype'] for c in short} == {A.F32, A.F64}          # a hue-last and a hue-not-last prefix
    cd = C.builder().cd
    for code, key in ((A.OP_BRIGHTNESS, 'brightness'), (A.OP_CONTRAST, 'contrast'), (A.OP_SATURATION, 'saturation'), (A.OP_HUE, 'hue')):
        deltas = {o[1] for c in cs for o in c['recipe']['ops'] if o[0] == code}
        assert {float(cd[key][0]), float(cd[key][1])} <= deltas, key             # both ends of the range the planner draws from
    full = [np.asarray(C.expected_canvas(c['name']), np.float64) for c in cs if len(c['recipe']['ops']) == 4]
    distinct = {a.tobytes() for a in full}
    assert len(distinct) >= 20, len(distinct)                                   # (orders that only swap two scalings may coincide)


def test_expand_stages_reach_every_wrap_class_in_float32_and_float64():
    seen = {A.F32: np.zeros(5, np.int64), A.F64: np.zeros(5, np.int64)}
    genuine64 = np.zeros(5, np.int64)
    for c in C.family('expand'):
        n = np.array(C.wrap_classes(C.stage(c['recipe'])))
        seen[c['dtype']] += n
        if c['dtype'] == A.F64 and c['stage'] != 'f64_dyadic':
            genuine64 += n
    for dt in (A.F32, A.F64):
        assert (seen[dt] > 0).all(), (C.DT_NAME[dt], dict(zip(C.WRAP_CLASSES, seen[dt])))
    # with matrices of _hue_matrix alone the float64 stage reaches every class but 'below 0 and integral'
    assert (genuine64[[0, 2, 3, 4]] > 0).all() and genuine64[1] == 0
    assert max(float(C.stage(c['recipe']).max()) for c in C.family('expand')) >= 512
    assert {c['placement'] for c in C.family('expand')} == {p[0] for p in C.PLACEMENTS}
    # the wrap itself, on the CPU: truncate toward zero, keep the low 8 bits
    for c in C.family('expand'):
        st = C.stage(c['recipe'])
        assert np.array_equal(st.astype(np.uint8), (np.trunc(st).astype(np.int64) & 255).astype(np.uint8))


def test_mixup_factors():
    f32 = np.float32
    blend = lambda f: f32(255) * f32(f) + f32(255) * f32(1.0 - f)             # float32 throughout, as the reference's array ops
    assert int(blend(C.F_254)) == 254 and blend(C.F_254) > 254.9999
    assert all(int(blend(f)) == 255 for f in (1e-3, 0.5, 0.999))
    assert float(f32(C.F_NOT_ONE)) + float(f32(1.0 - C.F_NOT_ONE)) != 1.0
    flat = {c['factor']: int(C.expected_canvas(c['name'])[0, 0, 0]) for c in C.family('mixup') if 'flat255' in c['name']}
    assert sorted(flat) == sorted(C.MIX_FACTORS) and 254 in flat.values() and 255 in flat.values()
    assert {c['to_rgb'] for c in C.family('mixup')} == {True, False}


def test_crop_windows():
    wins = {(c['window'], c['recipe']['flip']) for c in C.family('crop')}
    for flip in (False, True):
        assert ((1, 1), flip) in wins
        assert any(w[0] == 1 and w[1] > 1 and f == flip for w, f in wins) and any(w[1] == 1 and w[0] > 1 and f == flip for w, f in wins)
        assert {w[1] & 1 for w, f in wins if f == flip and w[1] > 1} == {0, 1}          # odd and even widths
    assert any(c['last_row'] and c['last_col'] for c in C.family('crop'))
    assert {c['recipe']['image'].shape[1] & 1 for c in C.family('crop')} == {0, 1}


def test_render_cases_cover_every_mode_dtype_and_size():
    cs = C.family('render')
    for S in C.RENDER_SIZES:
        assert {(c['recipe']['interp'], c['dtype']) for c in cs if c['S'] == S and 'up_13x17' in c['name']} == \
            {(i, d) for i in A.INTERPS for d in (A.U8, A.F32, A.F64)}
    assert [S % 64 != 0 for S in C.RENDER_SIZES] == [True] * 4 and sum(S > 64 for S in C.RENDER_SIZES) == 2
    assert sum(S % 4 != 0 for S in C.RENDER_SIZES) == 2
    modes = {(c['recipe']['resize']['mode'], c['recipe']['resize']['fixpt'], c['dtype']) for c in cs}
    assert modes == {(m, 0, d) for m in (A.MODE_NEAREST, A.MODE_SEP, A.MODE_AREA_FAST) for d in (A.U8, A.F32, A.F64)} | {(A.MODE_SEP, 1, A.U8)}
    assert {(c['recipe']['resize']['ix'], c['recipe']['resize']['iy']) for c in cs} == {(0, 0), (2, 2), (3, 3), (3, 2)}
    inside = [c for c in cs if c.get('inside_crop')]
    assert {(c['recipe']['interp'], c['dtype'], c['recipe']['flip']) for c in inside if c['leaves']} == \
        {(i, d, f) for i in (A.CUBIC, A.LANCZOS4) for d in (A.U8, A.F32, A.F64) for f in (False, True)}
    for c in C.family('overshoot'):
        c['promise'](c)                                 # (records the case's largest intermediate)
    worst = max(c['worst_accumulator'] for c in C.family('overshoot'))
    print('AUGMENT-CASES largest 8-bit accumulator: %d = %.3f of 2^31' % (worst, worst / 2.0 ** 31))
    assert worst < 2 ** 31


# ---------------------------------------------------------------------------------------------------------------------
# 2. the tables against the definitions (float64 canvases)

def _positions(n_dst, scale):
    return (np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5


def _keys(t, a=-0.75):
    """The cubic convolution kernel with parameter a."""
    t = np.abs(t)
    return np.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1, np.where(t < 2, ((a * t - 5 * a) * t + 8 * a) * t - 4 * a, 0.0))


def _lanczos(t, n=4):
    return np.where(np.abs(t) < n, np.sinc(t) * np.sinc(t / n), 0.0)


def _axis_matrix(interp, n_src, n_dst, shrink_area):
    """The [n_dst, n_src] float64 matrix one axis of the resize applies, border replicated."""
    scale = n_src / n_dst
    M = np.zeros((n_dst, n_src))
    d = np.arange(n_dst)

    def put(src, w):
        np.add.at(M, (np.broadcast_to(d[:, None], src.shape), np.clip(src, 0, n_src - 1)), w)

    if interp == A.NEAREST:
        put(np.minimum(np.floor(d * scale), n_src - 1).astype(np.int64)[:, None], np.ones((n_dst, 1)))
    elif interp == A.AREA and shrink_area:
        # the mean over the source interval [d * scale, (d + 1) * scale), each pixel weighted by its overlap with it
        for k in range(n_dst):
            lo, hi = k * scale, min((k + 1) * scale, n_src)
            for s in range(int(np.floor(lo)), int(np.ceil(hi))):
                M[k, s] += max(0.0, min(hi, s + 1) - max(lo, s)) / (hi - lo)
    elif interp in (A.LINEAR, A.AREA):
        if interp == A.LINEAR:
            pos = _positions(n_dst, scale)
            s = np.floor(pos)
            f = pos - s
        else:           # INTER_AREA when enlarging: pixel s = floor(d * scale) up to where its enlarged copy ends, then a ramp to s + 1
            s = np.floor(d * scale)
            f = (d + 1) - (s + 1) / scale
            f = np.where(f <= 0, 0.0, f - np.floor(f))
        s = s.astype(np.int64)
        put(np.stack([s, s + 1], 1), np.stack([1 - f, f], 1))
    else:
        pos = _positions(n_dst, scale)
        s = np.floor(pos).astype(np.int64)
        half = 2 if interp == A.CUBIC else 4
        k = np.arange(-half + 1, half + 1)
        t = pos[:, None] - (s[:, None] + k[None, :])
        w = _keys(t) if interp == A.CUBIC else _lanczos(t)
        if interp == A.LANCZOS4:
            w = w / w.sum(1, keepdims=True)             # OpenCV normalises the eight weights to sum 1
        put(s[:, None] + k[None, :], w)
    return M


def resize_by_definition(img, S, interp):
    """img float64 [h, w, 3] -> [S, S, 3]: rows first or columns first is the same in exact arithmetic."""
    h, w = img.shape[:2]
    shrink = w >= S and h >= S                          # INTER_AREA proper needs both axes to shrink (or keep their size)
    My, Mx = _axis_matrix(interp, h, S, shrink), _axis_matrix(interp, w, S, shrink)
    return np.einsum('yh,hwc,xw->yxc', My, img.astype(np.float64), Mx)


# measured on the CPU (profiles/augment_resize_definition.txt), relative to max|canvas|, per cv2.INTER_* code
MEASURED = {A.NEAREST: 0.0, A.LINEAR: 7.16e-07, A.AREA: 3.70e-08, A.CUBIC: 1.46e-06, A.LANCZOS4: 8.07e-07}
RESIZE_BOUND = {k: 4 * v for k, v in MEASURED.items()}


def _f64_render_cases(interp):
    return [c for c in C.family('render') if c['dtype'] == A.F64 and c['recipe']['interp'] == interp]


def _definition_error(c, plan=None):
    cv = np.array(C.expected_canvas(c['name']))
    assert cv.dtype == np.float64
    got = R.resize(cv, dict(resize=plan if plan is not None else c['recipe']['resize']))
    want = resize_by_definition(cv, c['S'], c['recipe']['interp'])
    assert got.shape == want.shape == (c['S'], c['S'], 3) and got.dtype == np.float64
    return float(np.abs(got - want).max() / np.abs(cv).max())


@pytest.mark.parametrize('interp', A.INTERPS)
def test_tables_equal_the_definitions(interp):
    cases = _f64_render_cases(interp)
    assert len(cases) >= 10
    errs = {c['name']: _definition_error(c) for c in cases}
    worst = max(errs, key=errs.get)
    print('AUGMENT-RESIZE-DEFINITION %s: %d cases, largest difference %.3e of max|canvas| (%s), bound %.3e'
          % (C.INTERP_NAME[interp], len(cases), errs[worst], worst, RESIZE_BOUND[interp]))
    assert errs[worst] <= RESIZE_BOUND[interp], (worst, errs[worst])


def _perturbed(plan, kind, n_src):
    """A copy of the plan with ONE entry wrong, at the middle output column / row: a weight (the row's largest) off by 2^-10, or
    a first-tap index off by one source pixel -- towards the inside, so that the border clamp cannot hide it."""
    p = copy.deepcopy(plan)
    mid = len(p[kind]) // 2
    if kind in ('xw', 'yw'):
        p[kind][mid, int(np.argmax(np.abs(p[kind][mid])))] += np.float32(2.0 ** -10)
    else:
        taps = {A.MODE_NEAREST: 1, A.MODE_AREA_FAST: p['ix' if kind == 'xfirst' else 'iy']}.get(p['mode'], p[kind[0] + 'w'].shape[1])
        p[kind][mid] += 1 if p[kind][mid] + taps < n_src else -1
    return p


@pytest.mark.parametrize('interp', A.INTERPS)
def test_the_definition_check_has_teeth(interp):
    """One weight off by 2^-10, or one first-tap index off by one: the comparison of test_tables_equal_the_definitions fails."""
    n_weight = n_index = 0
    for c in _f64_render_cases(interp):
        ch, cw = c['recipe']['crop'][2:]
        plan = c['recipe']['resize']
        if plan['mode'] == A.MODE_SEP:
            for kind in ('xw', 'yw'):
                assert _definition_error(c, _perturbed(plan, kind, cw if kind == 'xw' else ch)) > RESIZE_BOUND[interp], (c['name'], kind)
                n_weight += 1
        if cw > 1:
            assert _definition_error(c, _perturbed(plan, 'xfirst', cw)) > RESIZE_BOUND[interp], (c['name'], 'xfirst')
            n_index += 1
        if ch > 1:
            assert _definition_error(c, _perturbed(plan, 'yfirst', ch)) > RESIZE_BOUND[interp], (c['name'], 'yfirst')
            n_index += 1
    assert n_index >= 12 and (n_weight >= 12 or interp == A.NEAREST)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fixed-point and area tables

def test_fixed_point_tables_are_the_rounded_float_tables():
    n = 0
    for c in C.family('render') + C.family('overshoot') + C.family('crop'):
        r = c['recipe']
        p = r['resize']
        if not p['fixpt']:
            continue
        ch, cw = r['crop'][2:]
        q = A.resize_plan(ch, cw, r['fx'], r['fy'], r['interp'], A.F32)
        assert q['mode'] == A.MODE_SEP and q['fixpt'] == 0
        for k in ('xw', 'yw'):
            assert p[k].dtype == np.float32 and np.array_equal(p[k], np.rint(np.float32(2048) * q[k])), (c['name'], k)
            assert np.array_equal(p[k], np.rint(p[k])) and np.abs(p[k]).max() <= 32767
        assert np.array_equal(p['xfirst'], q['xfirst']) and np.array_equal(p['yfirst'], q['yfirst'])
        n += 1
    assert n >= 30


def test_area_table_rows_sum_to_one():
    n = 0
    for c in C.family('render'):
        p = c['recipe']['resize']
        if c['recipe']['interp'] != A.AREA or p['mode'] != A.MODE_SEP or p['fixpt']:
            continue
        for k in ('xw', 'yw'):
            K = p[k].shape[1]
            s = p[k].astype(np.float64).sum(1)
            assert np.abs(s - 1).max() <= (K + 1) * 2.0 ** -24, (c['name'], k, np.abs(s - 1).max())        # K roundings of weights <= 1
            assert (p[k] >= 0).all()
        n += 1
    assert n >= 6


# ---------------------------------------------------------------------------------------------------------------------
# 4. the target edge case (tests/test_gpu_augment.py scatters the same records on the device)

TARGET_S = 320
TARGET_IOU_THRESH = 0.7


def _level_square(g, mask):
    """(side s, offset d): s^2 is about the area of the level's first anchor."""
    a, b_ = g['anchors'][mask[0]]
    s = int(round((a * b_) ** 0.5))
    return s, max(1, s // 10)


def crowded_anchors(g):
    """The config's anchors with the first two of every level replaced by the near-square pair [s + d, s - d], [s - d, s + d].  Among
    the configs' own anchors no box of whole pixels has two equal best IoUs and none reaches 0.7 on two anchors (the best second
    IoU is 0.63).  A square box of side s has EXACTLY the same width / height IoU with both anchors of the pair (the products
    commute), about 0.83: the first must win the tie, and at iou_thresh = 0.7 the second claims the box as well."""
    an = [list(a) for a in g['anchors']]
    for mask in g['anchor_masks']:
        s, d = _level_square(g, mask)
        an[mask[0]], an[mask[1]] = [s + d, s - d], [s - d, s + d]
    return an


SQUARE_ROW = 7          # image 0, rows 7 ..: one square per level


def target_edge_boxes(g):
    """-> gt_bbox [2, 12, 4] (cx, cy, w, h normalised), gt_class [2, 12], gt_score [2, 12] as PadBox leaves them."""
    S = float(TARGET_S)
    below_one = np.nextafter(np.float32(1), np.float32(0))
    rows0 = [(0.5, 0.25, 100 / S, 100 / S, 3, 1.0),               # centre exactly on a cell boundary of every level
             (0.0, 0.0, 12 / S, 12 / S, 4, 0.5),                  # centre at 0
             (below_one, below_one, 45 / S, 52 / S, 5, 1.0),      # centre at the largest float32 below 1: the last cell, not one beyond
             (0.3, 0.3, 0.0, 0.2, 6, 1.0),                        # zero width: skipped
             (0.4, 0.4, 0.1, 0.1, 9, 0.0),                        # zero score: skipped
             (0.71, 0.33, 0.2, 0.3, 7, 0.3),                      # two boxes on one (anchor, cell): the later wins field by field,
             (0.715, 0.335, 0.21, 0.29, 8, 0.9)]                  # both class rows stay set
    assert len(rows0) == SQUARE_ROW
    for lv, mask in enumerate(g['anchor_masks']):
        s = _level_square(g, mask)[0]
        rows0.append((0.43 + 0.05 * lv, 0.6, s / S, s / S, 20 + lv, 1.0))
    rows1 = [(0.25, 0.75, 24 / S, 26 / S, 0, 1.0), (0.999, 0.001, 0.5, 0.6, 79, 0.25)]
    bb, cl, sc = np.zeros((2, 12, 4), np.float32), np.zeros((2, 12), np.int32), np.zeros((2, 12), np.float32)
    for n, rows in enumerate((rows0, rows1)):
        for k, row in enumerate(rows):
            bb[n, k], cl[n, k], sc[n, k] = row[:4], row[4], row[5]
    return bb, cl, sc


def _wh_iou(gw, gh, aw, ah):
    """IoU of (0, 0, gw, gh) and (0, 0, aw, ah) on numpy scalars: float32 box sides, float64 anchor sides."""
    if gw <= 0 or gh <= 0 or aw <= 0 or ah <= 0:
        return 0.0
    iw, ih = min(gw, aw), min(gh, ah)
    inter = iw * ih
    return inter / (gw * gh + aw * ah - inter)


def gt2yolo_loop(gt_bbox, gt_class, gt_score, anchors, anchor_masks, downsample_ratios, num_classes, size, iou_thresh):
    """Gt2YoloTarget one box at a time, from its documented semantics (ppyolo_hip/targets.py): the best of all anchors by width /
    height IoU (the first on a tie) claims the box on its level; with iou_thresh < 1 so does every other anchor of a level whose
    IoU exceeds it; boxes are written in order, so a later box overwrites the six fields and adds its class row."""
    out = []
    for mask, ds in zip(anchor_masks, downsample_ratios):
        grid = int(size / ds)
        t = np.zeros((gt_bbox.shape[0], len(mask), 6 + num_classes, grid, grid), np.float32)
        for n in range(gt_bbox.shape[0]):
            for b in range(gt_bbox.shape[1]):
                gx, gy, gw, gh = gt_bbox[n, b]
                score = gt_score[n, b]
                if gw <= 0 or gh <= 0 or score <= 0:
                    continue
                ious = [_wh_iou(gw, gh, a[0] / size, a[1] / size) for a in anchors]
                best, best_iou = -1, 0.0
                for a, v in enumerate(ious):
                    if v > best_iou:
                        best, best_iou = a, v
                gi, gj = int(gx * grid), int(gy * grid)
                for k, a in enumerate(mask):
                    if a != best and not (iou_thresh < 1 and ious[a] > iou_thresh):
                        continue
                    t[n, k, 0, gj, gi] = gx * grid - gi
                    t[n, k, 1, gj, gi] = gy * grid - gj
                    t[n, k, 2, gj, gi] = np.log(gw * size / anchors[a][0])
                    t[n, k, 3, gj, gi] = np.log(gh * size / anchors[a][1])
                    t[n, k, 4, gj, gi] = 2.0 - gw * gh
                    t[n, k, 5, gj, gi] = score
                    t[n, k, 6 + int(gt_class[n, b]), gj, gi] = 1.0
        out.append(t)
    return out


def target_edge_variants(g):
    """(name, anchors, iou_thresh) the edge boxes are run with."""
    return [('own anchors', [list(a) for a in g['anchors']], TARGET_IOU_THRESH), ('crowded anchors', crowded_anchors(g), TARGET_IOU_THRESH),
            ('crowded anchors, no threshold', crowded_anchors(g), 1.0)]


def _cells_of_class(levels, n, cls):
    """Where image n's class row `cls` is set -> [(level, anchor slot k, gj, gi)]."""
    return [(lv, int(k), int(j), int(i)) for lv, t in enumerate(levels) for k, j, i in np.argwhere(t[n, :, 6 + cls] == 1)]


@pytest.mark.parametrize('cfg_name', ['PPYOLO_2x_Config', 'PPYOLO_r18vd_Config'])
def test_target_edge_case_equals_the_per_box_loop(cfg_name):
    import config
    from ppyolo_hip import targets as T
    g = getattr(config, cfg_name)().gt2YoloTarget
    bb, cl, sc = target_edge_boxes(g)
    masks, dsr, nc = g['anchor_masks'], g['downsample_ratios'], g['num_classes']
    loops = {}
    for name, anchors, thr in target_edge_variants(g):
        want = gt2yolo_loop(bb, cl, sc, anchors, masks, dsr, nc, TARGET_S, thr)
        got = T.gt2yolo_target(bb, cl, sc, anchors, masks, dsr, nc, TARGET_S, thr)
        o, v = T.gt2yolo_records(bb, cl, sc, anchors, masks, dsr, nc, TARGET_S, thr)
        for lv, (a, b_) in enumerate(zip(got, want)):
            assert a.dtype == b_.dtype == np.float32 and a.shape == b_.shape
            assert np.array_equal(a, b_), (name, lv, int((a != b_).sum()))
        flat = np.zeros(sum(t.size for t in want), np.float32)
        assert len(np.unique(o)) == len(o)
        flat[o] = v
        assert np.array_equal(flat, np.concatenate([t.ravel() for t in want])), name
        loops[name] = want
    for name, want in loops.items():
        grids = [t.shape[-1] for t in want]
        on_edge, at_zero, below_one = (_cells_of_class(want, 0, c) for c in (3, 4, 5))
        assert on_edge and at_zero and below_one, name
        for lv, k, j, i in on_edge:
            assert (j, i) == (int(0.25 * grids[lv]), grids[lv] // 2) and want[lv][0, k, 0, j, i] == 0.0
            assert (want[lv][0, k, 1, j, i] == 0.0) == (grids[lv] % 4 == 0)
        for lv, k, j, i in at_zero:
            assert (j, i) == (0, 0) and not want[lv][0, k, :2, 0, 0].any() and want[lv][0, k, 5, 0, 0] == 0.5
        for lv, k, j, i in below_one:
            assert (j, i) == (grids[lv] - 1, grids[lv] - 1) and 0 < want[lv][0, k, 0, j, i] < 1
        assert not _cells_of_class(want, 0, 6) and not _cells_of_class(want, 0, 9)            # zero width, zero score
        first, later = _cells_of_class(want, 0, 7), _cells_of_class(want, 0, 8)
        assert first and first == later
        for lv, k, j, i in later:
            assert want[lv][0, k, 5, j, i] == np.float32(0.9) and want[lv][0, k, 4, j, i] == np.float32(2.0) - bb[0, 6, 2] * bb[0, 6, 3]
    # the tie: each level's square sits on the FIRST anchor of the pair alone, until the threshold lets the second in as well
    for lv in range(len(masks)):
        cls = int(cl[0, SQUARE_ROW + lv])
        alone = _cells_of_class(loops['crowded anchors, no threshold'], 0, cls)
        both = _cells_of_class(loops['crowded anchors'], 0, cls)
        assert [(c[0], c[1]) for c in alone] == [(lv, 0)] and sorted((c[0], c[1]) for c in both) == [(lv, 0), (lv, 1)]
        assert len(_cells_of_class(loops['own anchors'], 0, cls)) == 1
