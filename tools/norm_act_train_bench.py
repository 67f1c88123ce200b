"""Timings of the GroupNorm / AffineChannel training path (csrc/norm_act_train.hip, ppyolo_hip/train.py), in ONE process with the legs
alternating (report only, except the bn regression leg):

  kernels   at R50vd-608 batch 8, on the head's largest (76 x 76 x 256) and smallest (19 x 19 x 1024) GroupNorm maps:
            ppy_group_norm_train_f32 (three launches), ppy_group_norm_bwd_f32 (three launches) and a device-to-device copy of the
            same tensor, each replayed from a captured graph.  Floors: the backward's partial pass reads x and dy, its apply pass
            reads both again and writes dx -- five passes = 2.5 x a copy; the forward three = 1.5 x.
  step      TrainStep.step of PPYOLO_2x at 608 x 608, batch 8, freeze_at 5, synthetic weights and targets, with the head's norm
            'bn', 'gn' and 'affine_channel' (backbone bn).
  bn A/B    with --parent-lib: the bn step on this library and on the parent commit's, taking turns; MET when the two medians differ by
            no more than the windows' own spread.

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; min .. max beside it.

    python tools/norm_act_train_bench.py [--out profiles/norm_act_train_bench.txt] [--parent-lib PATH] [--seconds 1.0] [--rounds 5]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402
from jpeg_encode_bench import alternate, graph_of  # noqa: E402
from ppyolo_hip import _lib, ops as K  # noqa: E402


def other_library(path):
    """Another build of the library with this build's prototypes on every entry point it has."""
    L = ctypes.CDLL(path)
    for name, (res, args) in _lib._PROTOS.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'norm_act_train_bench.txt'))
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libppyolo_hip.so for the bn A/B leg")
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('norm_act_train_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('%s; batch %d; windows >= %.1f s, %d rounds, legs alternating' % (torch.cuda.get_device_name(0), a.bs, a.seconds, a.rounds))
    # ---- kernels ----
    legs, keep, shapes = {}, [], [(76, 76, 256), (19, 19, 1024)]
    for H, W, C in shapes:
        x, dy = torch.randn(a.bs, H, W, C, device='cuda'), torch.randn(a.bs, H, W, C, device='cuda')
        y, dx = torch.empty_like(x), torch.empty_like(x)
        gamma, beta = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')
        dg, db = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
        mean, rstd = torch.empty(a.bs * 32, dtype=torch.float64, device='cuda'), torch.empty(a.bs * 32, device='cuda')
        ws = K.group_norm_workspace(a.bs, 32, 'cuda')
        wsb = torch.empty(int(_lib.lib().ppy_group_norm_bwd_workspace_bytes(a.bs, H, W, C, 32)) // 4 + 2, device='cuda')
        xv, yv, dyv, dxv = K.View(x), K.View(y), K.View(dy), K.View(dx)
        keep.append((x, dy, y, dx, gamma, beta, dg, db, mean, rstd, ws, wsb))
        tag = '%dx%dx%d' % (H, W, C)

        def fwd(xv=xv, yv=yv, gamma=gamma, beta=beta, mean=mean, rstd=rstd, ws=ws):
            K.group_norm_train(xv, gamma, beta, 32, 1e-5, yv, mean, rstd, 'leaky', ws=ws)

        def bwd(xv=xv, dyv=dyv, dxv=dxv, gamma=gamma, beta=beta, mean=mean, rstd=rstd, dg=dg, db=db, wsb=wsb):
            K.group_norm_bwd(xv, mean, rstd, gamma, beta, 32, dyv, dxv, 'leaky', dgamma=dg, dbeta=db, ws=wsb)
        fwd()
        legs['gn fwd ' + tag] = graph_of(fwd)
        legs['gn bwd ' + tag] = graph_of(bwd)
        legs['copy   ' + tag] = graph_of(lambda x=x, y=y: y.copy_(x))
    res = alternate(legs, a.seconds, a.rounds)
    say('\nkernels: us per call (min .. max), GB/s at the floor traffic, time against the copy of the same tensor')
    for H, W, C in shapes:
        tag = '%dx%dx%d' % (H, W, C)
        nbytes = a.bs * H * W * C * 4
        cp = res['copy   ' + tag][0]
        for name, passes in (('gn fwd ', 3), ('gn bwd ', 5), ('copy   ', 2)):
            med, lo, hi = res[name + tag]
            say('  %s%-14s %8.1f us (%7.1f .. %7.1f)  %7.0f GB/s over %d passes of %.1f MB   %.2f x copy (floor %.2f x): %.2f x its floor'
                % (name, tag, med * 1e6, lo * 1e6, hi * 1e6, passes * nbytes / med / 1e9, passes, nbytes / 1e6, med / cp, passes / 2.0,
                   med / cp / (passes / 2.0)))
    del legs, keep
    torch.cuda.empty_cache()

    # ---- the training step ----
    from conftest import build_model
    from config import PPYOLO_2x_Config
    from ppyolo_hip import synth
    from ppyolo_hip.train import TrainStep
    from test_gpu_train_step import synth_targets          # a few positive cells per level, small boxes
    x = synth.synth_images(a.bs, a.size).cuda()
    legs, steps = {}, {}
    ours = _lib.lib()
    parent = other_library(a.parent_lib) if a.parent_lib else None

    def stepper(ts, gt, targets, library):
        def run():
            _lib._lib = library
            ts.step(x, gt, targets, 1e-4)
        return run
    for name, norm, library in (('head bn', 'bn', ours), ('head gn', 'gn', ours), ('head affine_channel', 'affine_channel', ours),
                                ('head bn, parent library', 'bn', parent)):
        if library is None:
            continue
        cfg = PPYOLO_2x_Config()
        cfg.head['norm_type'] = norm
        cfg.backbone['freeze_at'] = 5
        model, _ = build_model(cfg, 0, 'cuda')
        gt, targets = synth_targets(cfg, a.bs, a.size, 5)
        _lib._lib = library
        ts = TrainStep(model, cfg)
        steps[name] = ts
        legs[name] = stepper(ts, gt.cuda(), [t.cuda() for t in targets], library)
        for _ in range(3):
            legs[name]()
        torch.cuda.synchronize()
    res = alternate(legs, a.seconds, a.rounds)
    _lib._lib = ours
    say('\nstep: PPYOLO_2x %d x %d, batch %d, freeze_at 5, TrainStep.step (forward, loss, backward, SGD, EMA); ms per step (min .. max), img/s'
        % (a.size, a.size, a.bs))
    for name in legs:
        med, lo, hi = res[name]
        say('  %-28s %8.3f ms (%7.3f .. %7.3f)  %7.1f img/s' % (name, med * 1e3, lo * 1e3, hi * 1e3, a.bs / med))
    bn = res['head bn'][0]
    say('  gn / bn = %.3f, affine_channel / bn = %.3f (their outputs carry no tracked maximum: the head\'s convolutions, weight and data '
        'gradients run off the f16x2 tiles)' % (res['head gn'][0] / bn, res['head affine_channel'][0] / bn))
    if parent is not None:
        pm, plo, phi = res['head bn, parent library']
        spread = max(res['head bn'][2] - res['head bn'][1], phi - plo)
        say('  bn step, this library / parent library = %.4f; medians differ by %.3f ms, the windows spread over %.3f ms: %s'
            % (bn / pm, abs(bn - pm) * 1e3, spread * 1e3, 'MET' if abs(bn - pm) <= spread else 'MISSED'))
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
