"""Timings of the GroupNorm / Mish launches (csrc/norm_act.hip) and of the one-lane forward under the three norm types, in ONE
process with the legs alternating (report only: no number for these paths existed before):

  kernels   at R50vd-608 batch 8, on the 152 x 152 x 256 and 19 x 19 x 2048 maps: ppy_group_norm_f32 (three launches), ppy_mish_f32
            and a device-to-device copy of the same tensor, each replayed from a captured graph.  Floors: three passes over the
            tensor for GroupNorm (read, read, write), two for Mish and for the copy.
  forward   the one-lane forward (plan + decode, one hipGraph) of PPYOLO_2x at 608 x 608, batch 8, synthetic weights, with
            norm_type 'bn', 'affine_channel' and 'gn' in backbone and head; beside them 'bn' on the bf16x3 tiles (what the
            convolutions of a gn model fall back to: their inputs carry no tracked maximum) and the 'gn' ops of the gn plan alone,
            which splits the gn model's extra time into its launches and its convolutions.

Every figure is the median of `--rounds` windows of at least `--seconds`, the legs taking turns window by window; min .. max beside it.

    python tools/norm_act_bench.py [--out profiles/norm_act_bench.txt] [--bs 8] [--seconds 1.0] [--rounds 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'pytorch-ppyolo_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import torch  # noqa: E402
from jpeg_encode_bench import alternate, graph_of  # noqa: E402
from ppyolo_hip import ops as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'norm_act_bench.txt'))
    ap.add_argument('--bs', type=int, default=8)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('norm_act_bench needs the MI355X: a time taken anywhere else says nothing')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('%s; batch %d; windows >= %.1f s, %d rounds, legs alternating, graph replay' % (torch.cuda.get_device_name(0), a.bs, a.seconds, a.rounds))
    # ---- kernels ----
    legs, shapes = {}, [(152, 152, 256), (19, 19, 2048)]
    keep = []
    for H, W, C in shapes:
        x = torch.randn(a.bs, H, W, C, device='cuda')
        y, z = torch.empty_like(x), torch.empty_like(x)
        gamma, beta = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')
        ws = K.group_norm_workspace(a.bs, 32, 'cuda')
        xv, yv, zv = K.View(x), K.View(y), K.View(z)
        keep.append((x, y, z, gamma, beta, ws))
        tag = '%dx%dx%d' % (H, W, C)
        legs['gn   ' + tag] = graph_of(lambda xv=xv, yv=yv, gamma=gamma, beta=beta, ws=ws: K.group_norm(xv, gamma, beta, 32, 1e-5, yv, 'relu', ws=ws))
        legs['mish ' + tag] = graph_of(lambda zv=zv: K.mish(zv))          # (in place: the values settle at mish's fixed points, the time does not care)
        legs['copy ' + tag] = graph_of(lambda x=x, y=y: y.copy_(x))
    res = alternate(legs, a.seconds, a.rounds)
    say('\nkernels: us per call (min .. max), GB/s at the floor traffic, time against the copy of the same tensor')
    for H, W, C in shapes:
        tag = '%dx%dx%d' % (H, W, C)
        nbytes = a.bs * H * W * C * 4
        cp = res['copy ' + tag][0]
        for name, passes in (('gn   ', 3), ('mish ', 2), ('copy ', 2)):
            med, lo, hi = res[name + tag]
            say('  %s%-14s %8.1f us (%7.1f .. %7.1f)  %7.0f GB/s over %d passes of %.1f MB   %.2f x copy (floor %.2f x)'
                % (name, tag, med * 1e6, lo * 1e6, hi * 1e6, passes * nbytes / med / 1e9, passes, nbytes / 1e6, med / cp, passes / 2.0))
    del legs, keep
    torch.cuda.empty_cache()

    # ---- forward ----
    from conftest import build_model
    from config import PPYOLO_2x_Config
    from ppyolo_hip import synth
    from ppyolo_hip.engine import HipExecutor
    from ppyolo_hip.runtime import build_plan
    x = synth.synth_images(a.bs, a.size).cuda()
    ims = synth.synth_im_size(a.bs).cuda()
    legs, execs = {}, {}
    for name, norm, math in (('bn', 'bn', 'f16x2'), ('affine_channel', 'affine_channel', 'f16x2'), ('gn', 'gn', 'f16x2'), ('bn on bf16x3 tiles', 'bn', 'bf16x3')):
        cfg = PPYOLO_2x_Config()
        cfg.backbone['norm_type'] = cfg.head['norm_type'] = norm
        model, _ = build_model(cfg, 0, 'cuda')
        os.environ['PPYOLO_HIP_MATH'] = math
        ex = HipExecutor(build_plan(model, a.bs, a.size, a.size, torch.device('cuda')), 'cuda', use_graph=True)
        os.environ.pop('PPYOLO_HIP_MATH')
        ex.set_inputs(x, ims)
        ex.run()
        execs[name] = ex
        legs[name] = ex.run
    gx = execs['gn']
    gn_ops = [op for op in gx.plan.ops if op['op'] == 'gn']
    legs['gn ops of the gn plan alone'] = graph_of(lambda: [gx._run_op(op) for op in gn_ops])
    res = alternate(legs, a.seconds, a.rounds)
    say('\nforward: PPYOLO_2x %d x %d, batch %d, one lane, one hipGraph per step (plan + decode + NMS); ms per step (min .. max), img/s' % (a.size, a.size, a.bs))
    for name in legs:
        med, lo, hi = res[name]
        n_launch = sum(1 for op in execs[name].plan.ops) if name in execs else len(gn_ops)
        say('  %-28s %8.3f ms (%7.3f .. %7.3f)  %7.1f img/s   %d plan ops%s' % (name, med * 1e3, lo * 1e3, hi * 1e3, a.bs / med, n_launch,
                                                                              '' if name in execs else ' (x 3 launches)'))
    bn, af, gn, x3, alone = (res[k][0] for k in ('bn', 'affine_channel', 'gn', 'bn on bf16x3 tiles', 'gn ops of the gn plan alone'))
    say('  affine_channel / bn = %.4f (the same plan; bn windows span %.4f .. %.4f of their median)' % (af / bn, res['bn'][1] / bn, res['bn'][2] / bn))
    say('  gn / bn = %.3f: +%.3f ms, of which the gn launches alone %.3f ms (%.0f %%), the convolutions off the f16x2 tiles and out of every '
        'link %.3f ms (%.0f %%; bn on the bf16x3 tiles costs +%.3f ms over bn)' % (gn / bn, (gn - bn) * 1e3, alone * 1e3, 100 * alone / (gn - bn),
                                                                                   (gn - bn - alone) * 1e3, 100 * (gn - bn - alone) / (gn - bn), (x3 - bn) * 1e3))
    say('  (the gn model\'s shapes have no entry in the measured tile table where they differ from the bn plan\'s: those layers run on the library\'s own choice)')
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
