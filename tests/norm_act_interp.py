"""tests/plan_interp.py's CPU interpreter with the two ops of the GroupNorm / Mish path: a plan of a gn / af / mish model is
replayed with torch reference ops (tests/norm_act_ref.py), which checks the emission -- residual after the norm, channel-sliced
and upsampled destinations, the in-place Mish -- without a device."""
import torch.nn.functional as F

import norm_act_ref as R
from plan_interp import CpuPlanRunner


class NormActPlanRunner(CpuPlanRunner):
    def _run(self, op, x_in):
        t = op['op']
        if t == 'gn':
            x = self.get(op['x']).permute(0, 3, 1, 2)
            y = R.group_norm(x, op['scale'], op['shift'], op['groups'], op['eps'])
            if op['res'] is not None:
                y = y + self.get(op['res']).permute(0, 3, 1, 2)
            y = R.act(y, op['act'])
            if op['ups']:
                y = F.interpolate(y, scale_factor=2, mode='nearest')
            self.put(op['y'], y.permute(0, 2, 3, 1))
        elif t == 'mish':
            self.put(op['x'], R.mish(self.get(op['x'])))
        else:
            CpuPlanRunner._run(self, op, x_in)
