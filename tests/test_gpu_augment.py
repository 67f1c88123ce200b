"""Training batches on the device (ppyolo_hip/augment.py, csrc/augment.hip).  The canvas kernel is pinned to the reference
(g19_augment); the render kernel is compared bit for bit with the CPU restatement tests/augment_ref.py; the target kernel with
targets.gt2yolo_target; the builder with the CPU chain and in the reference's training call.  The hand-built edge recipes are
in tests/test_gpu_augment_edges.py.

What pins the restatement's resize: the planner's coefficient tables are checked against the interpolations' definitions in
float64, to the measured bound of tests/test_augment_cases.py (profiles/augment_resize_definition.txt); the 8-bit tables are
the rounded float tables; the restated 8-bit CUBIC equals oracle/preprocess_oracle.py.  NOT pinned: OpenCV's own rounding
inside its scalar templates (work types, accumulation order, the 8-bit and integer-scale AREA roundings), which only cv2 could
confirm and cv2 is not installed here."""
import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import build_train_model
from config import PPYOLO_2x_Config, PPYOLO_r18vd_Config
from ppyolo_hip import augment as A, ops, targets as T
from ppyolo_hip._lib import PPYoloHipError, lib
from test_augment_cases import TARGET_S, gt2yolo_loop, target_edge_boxes, target_edge_variants
from test_augment_plan import golden_batches, plan_batch

pytestmark = pytest.mark.gpu
DT = {A.U8: np.uint8, A.F32: np.float32, A.F64: np.float64}


def test_canvas_kernel_equals_the_reference(golden):
    g = golden('g19_augment')
    b = A.TrainBatchBuilder(PPYOLO_2x_Config())
    n = 0
    for seed, shape, samples, gold, _ in golden_batches(g):
        _, (recipes, _, _, _) = plan_batch(b, seed, samples)
        for r, gd in zip(recipes, gold):
            got = b.canvas(r).cpu().numpy()
            want = gd['canvas']
            assert got.dtype == want.dtype and got.shape == want.shape
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)
                print('canvas differs (seed %d):' % seed, got[bad][:8], want[bad][:8])
                # only a hue-last float64 canvas may differ, by one float64 ulp
                assert want.dtype == np.float64, seed
                assert np.all(np.abs(got[bad] - want[bad]) <= np.spacing(np.abs(want[bad]))), seed
            n += 1
    assert n >= 40


def _recipe(img, S, interp, dtype, flip=False):
    ops_ = {A.U8: [], A.F32: [(A.OP_CONTRAST, 1.2345, None), (A.OP_BRIGHTNESS, -3.25, None)],
            A.F64: [(A.OP_SATURATION, 0.8, None), (A.OP_HUE, 7.0, A._hue_matrix(7.0))]}[dtype]
    h, w = img.shape[:2]
    return dict(image=img, mix_image=None, factor=None, ops=ops_, color_dtype=dtype, canvas_dtype=dtype, expand=None,
                fill=np.array([123, 116, 103], np.uint8), crop=(0, 0, h, w), flip=flip, interp=interp, fx=S / w, fy=S / h,
                resize=A.resize_plan(h, w, S / w, S / h, interp, dtype))


def _render(b, recipes, S):
    blob, _ = A.pack_batch(recipes, True, np.zeros(0), np.zeros(0, np.float32), None, None, None)
    dev = torch.from_numpy(blob).cuda()
    out = torch.full((len(recipes), 3, S, S), float('nan'), device='cuda')
    ops.augment_render(dev, len(recipes), S, torch.from_numpy(b.lut_np).cuda(), b.mean, b.std, out)
    return out.cpu().numpy()


@pytest.mark.parametrize('interp', [A.NEAREST, A.LINEAR, A.AREA, A.CUBIC, A.LANCZOS4])
def test_render_kernel_equals_the_cpu_restatement(interp):
    """Every interpolation x {uint8, float32, float64} canvas x up / down / integer scales, S 320 ... 608."""
    b = A.TrainBatchBuilder(PPYOLO_2x_Config())
    rng = np.random.RandomState(interp)
    for (h, w), S in (((304, 304), 608), ((640, 640), 320), ((960, 640), 320), ((500, 700), 416), ((150, 200), 352),
                      ((611, 97), 608), ((320, 320), 320)):
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        recipes = [_recipe(img, S, interp, dt, flip=dt == A.F32) for dt in (A.U8, A.F32, A.F64)]
        got = _render(b, recipes, S)
        want = R.images(recipes, b.mean, b.std)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (interp, h, w, S, k, np.abs(got[k] - want[k]).max())


@pytest.mark.parametrize('cfgc', [PPYOLO_2x_Config, PPYOLO_r18vd_Config])
def test_target_kernel_equals_gt2yolo_target(cfgc):
    g = cfgc().gt2YoloTarget
    bb, cl, sc = T.synth_ground_truth(6, 9)
    bb[2, 10:14] = bb[2, 3]                                 # four boxes on one (anchor, cell): later wins, classes stay
    cl[2, 10:14] = [5, 6, 7, 5]
    sc[2, 10:14] = [0.3, 0.4, 0.5, 0.6]
    for S in (320, 608):
        ref = T.gt2yolo_target(bb, cl, sc, g['anchors'], g['anchor_masks'], g['downsample_ratios'], 80, S)
        o, v = T.gt2yolo_records(bb, cl, sc, g['anchors'], g['anchor_masks'], g['downsample_ratios'], 80, S)
        blob, lay = A.pack_batch([], True, o, v, None, None, None)
        dev = torch.from_numpy(blob).cuda()
        flat = torch.full((sum(r.size for r in ref),), 7.0, device='cuda')
        ops.augment_targets(flat, dev, lay['toff'], lay['tval'], len(o))
        assert torch.equal(flat.cpu(), torch.from_numpy(np.concatenate([r.ravel() for r in ref])))


@pytest.mark.parametrize('cfgc', [PPYOLO_2x_Config, PPYOLO_r18vd_Config])
def test_target_kernel_on_the_edge_boxes(cfgc):
    """Centres on a cell boundary, at 0 and at the largest float32 below 1, an exact tie of two anchors, a zero-width and a
    zero-score box, iou_thresh = 0.7 with one box on two anchors of a level (tests/test_augment_cases.py builds them and checks
    the same on the CPU): the records scattered by the device equal gt2yolo_target, and both equal the per-box loop."""
    g = cfgc().gt2YoloTarget
    bb, cl, sc = target_edge_boxes(g)
    for name, anchors, thr in target_edge_variants(g):
        args = (bb, cl, sc, anchors, g['anchor_masks'], g['downsample_ratios'], g['num_classes'], TARGET_S, thr)
        ref = T.gt2yolo_target(*args)
        o, v = T.gt2yolo_records(*args)
        blob, lay = A.pack_batch([], True, o, v, None, None, None)
        dev = torch.from_numpy(blob).cuda()
        flat = torch.full((sum(r.size for r in ref),), 7.0, device='cuda')
        ops.augment_targets(flat, dev, lay['toff'], lay['tval'], len(o))
        got = flat.cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, np.concatenate([r.ravel() for r in ref])), name
        assert np.array_equal(got, np.concatenate([r.ravel() for r in gt2yolo_loop(*args)])), name


def _cpu_chain(b, recipes, bb, cl, sc, S):
    t = T.gt2yolo_target(bb, cl, sc, b.anchors, b.anchor_masks, b.downsample_ratios, b.num_classes, S)
    return R.images(recipes, b.mean, b.std), t


def test_builder_equals_the_cpu_chain_and_is_deterministic(golden):
    g = golden('g19_augment')
    b = A.TrainBatchBuilder(PPYOLO_2x_Config())
    for seed, shape, samples, gold, _ in golden_batches(g)[:6]:
        np.random.seed(seed)
        S = np.random.choice(PPYOLO_2x_Config().randomShape['sizes'])
        out = b(samples, S)
        torch.cuda.synchronize()
        _, (recipes, bb, cl, sc) = plan_batch(b, seed, samples)
        im, tg = _cpu_chain(b, recipes, bb, cl, sc, S)
        assert np.array_equal(out['images'].cpu().numpy(), im), seed
        for i, t in enumerate(tg):
            assert torch.equal(out['target%d' % i].cpu(), torch.from_numpy(t)), (seed, i)
        assert np.array_equal(out['gt_bbox'].cpu().numpy(), bb) and np.array_equal(out['gt_class'].cpu().numpy(), cl)
        assert np.array_equal(out['gt_score'].cpu().numpy(), sc)
        assert out['gt_class'].dtype == torch.int32 and out['images'].shape == (len(samples), 3, S, S)
        np.random.seed(seed)
        S2 = np.random.choice(PPYOLO_2x_Config().randomShape['sizes'])
        again = b(samples, S2)
        assert torch.equal(again['images'], out['images']) and torch.equal(again['target2'], out['target2'])


def test_bad_arguments_return_errors():
    L = lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    out = torch.zeros(3 * 8 * 8, device='cuda')
    lut = torch.zeros(3, 256, device='cuda')
    import ctypes
    ms = (ctypes.c_double * 6)(0, 0, 0, 1, 1, 1)
    s = torch.cuda.current_stream().cuda_stream
    assert L.ppy_augment_render_f32(None, 4096, 1, 8, lut.data_ptr(), ms, 1, out.data_ptr(), s) != 0
    assert L.ppy_augment_render_f32(buf.data_ptr(), 100, 1, 8, lut.data_ptr(), ms, 1, out.data_ptr(), s) != 0   # blob too small
    assert L.ppy_augment_render_f32(buf.data_ptr(), 4096, 0, 8, lut.data_ptr(), ms, 1, out.data_ptr(), s) != 0
    assert L.ppy_augment_canvas(buf.data_ptr(), 4096, 0, 8, 8, 5, out.data_ptr(), s) != 0
    assert L.ppy_augment_targets_f32(out.data_ptr(), 192, None, None, 3, s) != 0
    # a descriptor of zeros is invalid: the kernels skip it and write nothing
    out.fill_(5.0)
    assert L.ppy_augment_render_f32(buf.data_ptr(), 4096, 1, 8, lut.data_ptr(), ms, 1, out.data_ptr(), s) == 0
    assert L.ppy_augment_canvas(buf.data_ptr(), 4096, 0, 8, 8, 0, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


def _batch(seed, n, S, b):
    rng = np.random.RandomState(seed)
    samples = []
    for k in range(n):
        h, w = int(rng.randint(200, 480)), int(rng.randint(200, 480))
        G = int(rng.randint(1, 12))
        x1, y1 = rng.uniform(0, w - 40, G), rng.uniform(0, h - 40, G)
        box = np.stack([x1, y1, x1 + rng.uniform(20, 40, G), y1 + rng.uniform(20, 40, G)], 1).astype(np.float32)
        samples.append(dict(image=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), h=h, w=w, gt_bbox=box,
                            gt_class=rng.randint(0, 80, (G, 1)).astype(np.int32), gt_score=np.ones((G, 1), np.float32),
                            is_crowd=np.zeros((G, 1), np.int32)))
    np.random.seed(seed)
    return samples


def test_reference_training_call_fed_by_the_builder():
    """model(images, None, False, gt_bbox, gt_class, gt_score, targets) on the builder's batch gives the losses of the same
    call on the CPU chain's tensors; then two optimiser steps at two sizes (320, 416) stay finite."""
    cfg = PPYOLO_r18vd_Config()
    b = A.TrainBatchBuilder(cfg)
    m = build_train_model(cfg, 0, 'cuda')
    m.head.set_dropblock(is_test=True)
    samples = _batch(5, 2, 320, b)
    state = np.random.get_state()
    out = b(samples, 320)
    np.random.set_state(state)
    recipes, bb, cl, sc = b.plan(samples, 320)
    im, tg = _cpu_chain(b, recipes, bb, cl, sc, 320)
    C = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    l_dev = m(out['images'], None, False, out['gt_bbox'], out['gt_class'], out['gt_score'], [out['target0'], out['target1']])
    l_cpu = m(C(im), None, False, C(bb), C(cl), C(sc), [C(t) for t in tg])
    for k in l_dev:
        assert torch.equal(l_dev[k].detach(), l_cpu[k].detach()), k
    groups = []
    m.add_param_group(groups, 1e-4, 5e-4)
    opt = torch.optim.SGD(groups, lr=1e-4, momentum=0.9, weight_decay=5e-4)
    for it, S in enumerate((320, 416)):
        batch = b(_batch(20 + it, 2, S, b), S)
        losses = m(batch['images'], None, False, batch['gt_bbox'], batch['gt_class'], batch['gt_score'],
                   [batch['target0'], batch['target1']])
        total = sum(losses.values())
        opt.zero_grad()
        total.backward()
        opt.step()
        assert np.isfinite(float(total.detach())), (S, {k: float(v) for k, v in losses.items()})
