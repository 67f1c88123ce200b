"""The training-batch planner (ppyolo_hip/augment.py) against the reference's own training reader (g19_augment, made by
tools/make_goldens.py g19 with the reference's transform classes): every draw, recipe, final box array and the final
np.random state, bit for bit; the CPU restatement's canvases and normalisation against the reference's.  Of the resize,
the 8-bit CUBIC restatement is checked here against oracle/preprocess_oracle.py; tests/test_augment_cases.py checks the
coefficient tables against the interpolations' definitions (what stays unpinned without cv2: see tests/augment_ref.py)."""
import numpy as np
import pytest

import augment_ref as R
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from oracle import preprocess_oracle as po
from ppyolo_hip import augment as A
from ppyolo_hip._lib import PPYoloHipError


def golden_batches(g):
    """-> list of (seed, shape, samples, per-sample golden dict, state)."""
    out = []
    for nb in range(int(g['n_batches'])):
        p = 'b%d_' % nb
        samples, gold = [], []
        for k in range(int(g['batch_size'])):
            q = p + 's%d_' % k

            def rec(nm):
                im = g[q + nm + '_img']
                return dict(image=im, h=im.shape[0], w=im.shape[1],
                            **{k2: g[q + nm + '_' + k2] for k2 in ('gt_bbox', 'gt_class', 'gt_score', 'is_crowd')})
            s = rec('a')
            if q + 'b_img' in g:
                s['mixup'] = rec('b')
            samples.append(s)
            gold.append({k2: g[q + k2] for k2 in ('canvas', 'draws', 'out_gt_bbox', 'out_gt_class', 'out_gt_score', 'normalized')
                         if q + k2 in g})
        out.append((int(g[p + 'seed']), int(g[p + 'shape']), samples, gold, (g[p + 'state_keys'], g[p + 'state_pos'])))
    return out


def plan_batch(builder, seed, samples):
    np.random.seed(seed)
    shape = np.random.choice(PPYOLO_2x_Config().randomShape['sizes'])      # train.py:90, before get_samples
    return shape, builder.plan(samples, shape)


def test_plan_reproduces_the_reference_reader(golden):
    g = golden('g19_augment')
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    seen = set()
    for seed, shape, samples, gold, (keys, pos) in golden_batches(g):
        got_shape, (recipes, bb, cl, sc) = plan_batch(b, seed, samples)
        assert got_shape == shape
        st = np.random.get_state()
        assert np.array_equal(st[1], keys) and st[2] == int(pos[0]), 'np.random state after the batch differs'
        for r, gd, k in zip(recipes, gold, range(len(recipes))):
            fx, fy, interp = gd['draws']
            assert (r['interp'], r['fx'], r['fy']) == (int(interp), fx, fy), (seed, k)
            assert np.array_equal(bb[k], gd['out_gt_bbox']) and bb.dtype == np.float32, (seed, k)
            assert np.array_equal(cl[k], gd['out_gt_class']) and cl.dtype == np.int32, (seed, k)
            assert np.array_equal(sc[k], gd['out_gt_score']) and sc.dtype == np.float32, (seed, k)
            assert {A.U8: np.uint8, A.F32: np.float32, A.F64: np.float64}[r['canvas_dtype']] == gd['canvas'].dtype
            assert (r['crop'][2], r['crop'][3]) == gd['canvas'].shape[:2]
            seen.add(('interp', r['interp']))
            seen.add(('dtype', r['canvas_dtype']))
            seen.add('mixup' if r['factor'] is not None else 'no_mixup')
            seen.add('expand' if r['expand'] is not None else 'no_expand')
            seen.add('flip' if r['flip'] else 'no_flip')
            seen.add('crop' if r['crop'][:2] != (0, 0) or r['crop'][2:] != (r['expand'] or (0, 0))[:2] else 'full')
            seen.update(('op', o[0]) for o in r['ops'])
            if r['ops'] and r['ops'][-1][0] == A.OP_HUE:
                seen.add('hue_last')
            if int((np.abs(bb[k]).sum(1) > 0).sum()) == 50:
                seen.add('50_boxes')
    want = {('interp', i) for i in range(5)} | {('dtype', d) for d in range(3)} | {('op', o) for o in range(4)}
    want |= {'mixup', 'no_mixup', 'expand', 'no_expand', 'flip', 'no_flip', 'hue_last', '50_boxes'}
    assert want <= seen, want - seen


def test_cpu_canvas_and_normalisation_equal_the_reference(golden):
    """augment_ref.canvas (the reference's numpy ops on the planned recipe) equals the reference's pre-resize image; the
    float canvases' NormalizeImage + Permute equal the reference's."""
    g = golden('g19_augment')
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    n = 0
    for seed, shape, samples, gold, _ in golden_batches(g):
        _, (recipes, _, _, _) = plan_batch(b, seed, samples)
        for r, gd in zip(recipes, gold):
            cv = R.canvas(r)
            assert cv.dtype == gd['canvas'].dtype and np.array_equal(cv, gd['canvas']), seed
            if 'normalized' in gd:
                assert np.array_equal(R.normalize(gd['canvas'], b.mean, b.std), gd['normalized'])
                n += 1
    assert n > 0


def test_restated_cubic_u8_equals_the_preprocess_oracle():
    rng = np.random.RandomState(3)
    for h, w, S in ((37, 51, 320), (480, 640, 416), (700, 300, 352)):
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        r = dict(resize=A.resize_plan(h, w, S / w, S / h, A.CUBIC, A.U8))
        assert np.array_equal(R.resize(img, r), po.resize_cubic_u8(img, S / w, S / h))


def test_new_config_attributes_equal_the_reference(golden):
    g = golden('g19_augment')
    c, r = PPYOLO_2x_Config(), PPYOLO_r18vd_Config()
    for k in ('mixupImage', 'colorDistort', 'randomExpand', 'randomCrop', 'randomFlipImage', 'normalizeBox', 'padBox',
              'bboxXYXY2XYWH', 'randomShape', 'gt2YoloTarget', 'decodeImage'):
        assert repr(sorted(getattr(c, k).items())) == str(g['cfg_2x_' + k]), k
    assert repr(sorted(r.gt2YoloTarget.items())) == str(g['cfg_r18vd_gt2YoloTarget'])
    assert c.sample_transforms_seq == [str(v) for v in g['cfg_sample_transforms_seq']] == r.sample_transforms_seq
    assert c.batch_transforms_seq == [str(v) for v in g['cfg_batch_transforms_seq']] == r.batch_transforms_seq
    assert c.context == {'fields': ['image']}                  # the inference harness's context is unchanged


@pytest.mark.parametrize('attr,key,val', [('decodeImage', 'with_cutmix', True), ('colorDistort', 'hsv_format', True),
                                          ('colorDistort', 'random_channel', True), ('colorDistort', 'random_apply', False),
                                          ('randomShape', 'resize_box', True), ('randomCrop', 'is_mask_crop', True)])
def test_unsupported_settings_raise(attr, key, val):
    cfg = PPYOLO_2x_Config()
    getattr(cfg, attr)[key] = val
    with pytest.raises(PPYoloHipError):
        A.TrainBatchBuilder(cfg, device='cpu')


def test_unsupported_records_and_sizes_raise():
    b = A.TrainBatchBuilder(PPYOLO_2x_Config(), device='cpu')
    im = np.zeros((40, 30, 3), np.uint8)
    rec = dict(image=im, h=40, w=30, gt_bbox=np.zeros((0, 4), np.float32), gt_class=np.zeros((0, 1), np.int32),
               gt_score=np.zeros((0, 1), np.float32), is_crowd=np.zeros((0, 1), np.int32))
    with pytest.raises(PPYoloHipError):
        b.plan([dict(rec, gt_poly=[[1, 2, 3]])], 320)
    with pytest.raises(PPYoloHipError):
        b.plan([dict(rec, image=im.astype(np.float32))], 320)
