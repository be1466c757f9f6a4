"""The layer-wise trust ratio (LARS / LARC) as a plain-torch wrapper around torch.optim.SGD: the reference the HipLARS
tests and tools/microbench/lars_step_bench.py compare with.  Written from the formula in include/sfhip.h
(sf_lars_ratios), not from any implementation; usable in float64 on the CPU and in float32 on the GPU.

Per parameter with a gradient, wd and lr its group's, pn = ||p||, gn = ||g||:
    the group has apply_LARS False, or the parameter is 1-D under ignore_1d_param:   r = 1, wd_t = wd
    a norm that is not finite:                                                       r = 1, wd_t = wd
    pn != 0 and gn != 0:     r = trust * pn / (gn + pn * wd + eps);  with clip: r = min(r / lr, 1);  wd_t = wd
    a zero norm:                                                                     r = 1, wd_t = 0
then  p.grad += wd_t * p;  p.grad *= r  and torch.optim.SGD's step with the group's weight_decay set to 0 around it."""
import math

import torch


class LarsRef(object):
    def __init__(self, optim, trust_coefficient=0.02, clip=True, eps=1e-8, ignore_1d_param=False):
        self.optim = optim
        self.trust_coefficient, self.clip, self.eps = float(trust_coefficient), bool(clip), float(eps)
        self.ignore_1d_param = bool(ignore_1d_param)

    @property
    def param_groups(self):
        return self.optim.param_groups

    @property
    def state(self):
        return self.optim.state

    def ratio(self, p, group):
        """(r, wd_t) of one parameter as Python floats; the norms are taken in the parameter's own dtype."""
        wd, lr = float(group["weight_decay"]), float(group["lr"])
        if not group.get("apply_LARS", True) or (self.ignore_1d_param and p.dim() <= 1):
            return 1.0, wd
        pn, gn = float(torch.norm(p.detach())), float(torch.norm(p.grad.detach()))
        if not (math.isfinite(pn) and math.isfinite(gn)):
            return 1.0, wd
        if pn == 0.0 or gn == 0.0:
            return 1.0, 0.0
        r = self.trust_coefficient * pn / (gn + pn * wd + self.eps)
        if self.clip:
            r = min(r / lr, 1.0)
        return r, wd

    def ratios(self):
        """[(r, wd_t)] of every parameter that has a gradient, group by group — sf_lars_ratios' table order."""
        return [self.ratio(p, g) for g in self.param_groups for p in g["params"] if p.grad is not None]

    @torch.no_grad()
    def step(self):
        saved = []
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                r, wd_t = self.ratio(p, g)
                p.grad.add_(p, alpha=wd_t)
                p.grad.mul_(r)
            saved.append(g["weight_decay"])
            g["weight_decay"] = 0
        self.optim.step()
        for g, wd in zip(self.param_groups, saved):
            g["weight_decay"] = wd
