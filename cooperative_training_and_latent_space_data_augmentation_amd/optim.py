"""Flat multi-tensor Adam: ONE kernel launch per network updates every parameter (the reference uses one
`optim.Adam(model.parameters(), lr)` per network: model.py:774-785).  State dicts are laid out like torch.optim.Adam's
(`state` keyed by parameter index with `step`, `exp_avg`, `exp_avg_sq`; one param group) so upstream `_optim.pth` /
snapshot files round-trip.

The optimizer tail (opt-in, `FlatAdam.configure`): the learning rate, the clip factor of the global gradient norm and the decision to
skip a step whose gradient is not finite are read by the kernel from the solver's device control record (ops.optim_control /
ops.grad_norm), and the EMA shadow of the weights is updated in the same pass (ops.adam_tail).  `grad_norm_host` and `adam_tail_host`
are the definitions the kernels are tested against."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops


class FlatAdam:
    def __init__(self, net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        self.net = net
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False)
        self.param_groups = [dict(self.defaults, params=list(net.parameters()))]
        self.exp_avg = torch.zeros_like(net._flat_data)
        self.exp_avg_sq = torch.zeros_like(net._flat_data)
        self.step_count = 0
        # optimizer tail: off until configure() hands over the solver's control record
        self.ctrl, self.net_index = None, 0
        self.ema = None                      # flat shadow of the weights, laid out like exp_avg
        self.num_updates = 0                 # EMA updates issued so far (host count: a step the device skips is counted too)

    def configure(self, ctrl, net_index: int, use_ema: bool = False):
        """Route step() through the tail kernel: `ctrl` = the solver's control record (ops.optim_ctrl), `net_index` = this network's
        lr slot in it; use_ema allocates the shadow, initialised to the weights.  configure(None, 0) goes back to the plain launch."""
        self.ctrl, self.net_index = ctrl, int(net_index)
        if ctrl is None or not use_ema:
            self.ema = None
        elif self.ema is None:
            self.ema = self.net._flat_data.detach().clone()
            self.num_updates = 0

    def zero_grad(self, set_to_none: bool = False):
        self.net.zero_grad()                 # gradients are views of one flat buffer that is never re-allocated

    def step(self, closure=None, grad_scale: float = 1.0, state=None):
        """`state`: device int64[3] whose [2] holds the (already advanced) step count -- HIP-graph capture, where the host-side
        count must not be a launch argument; the host count is still advanced as the mirror that state dicts report.
        Like torch.optim.Adam (which skips parameters whose `.grad` is None) the step is skipped when no backward pass has written
        this network's gradient since the last zero_grad() (set_to_none semantics of torch >= 2.0)."""
        if not self.net._grad_written:
            return
        g = self.param_groups[0]
        self.step_count += 1
        if self.ctrl is not None:            # lr, clip and the skip decision come from the control record
            ops.adam_tail(self.net._flat_data, self.net._flat.grad, self.exp_avg, self.exp_avg_sq, self.ema, g["betas"][0], g["betas"][1],
                          g["eps"], self.step_count, grad_scale, self.ctrl, self.net_index, state=state)
            if self.ema is not None:
                self.num_updates += 1
            self.net.weights_changed()
            return
        ops.adam_step(self.net._flat_data, self.net._flat.grad, self.exp_avg, self.exp_avg_sq, g["lr"], g["betas"][0],
                      g["betas"][1], g["eps"], self.step_count, grad_scale, state=state)
        self.net.weights_changed()

    def _views(self, flat):
        net = self.net
        return [flat[net._poff[n]:net._poff[n] + p.numel()].view(p.shape) for n, p in net.named_parameters()]

    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i, (m, v) in enumerate(zip(self._views(self.exp_avg), self._views(self.exp_avg_sq))):
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m.detach().cpu().clone(),
                            "exp_avg_sq": v.detach().cpu().clone()}
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g["params"] = list(range(len(self.param_groups[0]["params"])))
        sd = {"state": state, "param_groups": [g]}
        if self.ema is not None:             # new keys, present only with EMA on
            sd["ema"] = [e.detach().cpu().clone() for e in self._views(self.ema)]
            sd["num_updates"] = int(self.num_updates)
        return sd

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        for k in ("lr", "betas", "eps"):
            if k in g:
                self.param_groups[0][k] = tuple(g[k]) if k == "betas" else g[k]
        ms, vs = self._views(self.exp_avg), self._views(self.exp_avg_sq)
        self.step_count = 0
        for i, st in sd["state"].items():
            ms[int(i)].copy_(st["exp_avg"])
            vs[int(i)].copy_(st["exp_avg_sq"])
            self.step_count = int(float(st["step"]))
        if self.ema is not None:
            if "ema" in sd:
                for dst, src in zip(self._views(self.ema), sd["ema"]):
                    dst.copy_(src)
                self.num_updates = int(sd.get("num_updates", 0))
            else:                            # a file written without EMA: the shadow starts from the weights, as a fresh one does
                self.ema.copy_(self.net._flat_data)
                self.num_updates = 0


def ema_decay_at(decay: float, num_updates) -> float:
    """The decay of EMA update number `num_updates` (1-based; None = no warm-up): min(decay, (1 + n) / (10 + n))."""
    return float(decay) if num_updates is None else min(float(decay), (1 + num_updates) / (10 + num_updates))


# ---------------------------------------------------------------------------------------------- host statements (fp64)
def grad_norm_host(grads, grad_scale: float = 1.0, max_norm: float = 0.0, guard: bool = False):
    """-> (sumsq, norm, clip, finite) of flat gradient buffers as ctl_grad_norm defines them, in fp64: norm = grad_scale * sqrt(sum g^2);
    clip = min(1, max_norm / (norm + 1e-6)) when max_norm > 0 and the norm is finite, else 1.  `guard` does not enter the four values
    (it decides whether a non-finite step is skipped); it is taken so that call sites read like the kernel's."""
    sumsq = 0.0
    for g in grads:
        a = np.asarray(g.detach().cpu() if torch.is_tensor(g) else g, dtype=np.float64).ravel()
        with np.errstate(over="ignore", invalid="ignore"):
            sumsq += float(np.sum(a * a))
    norm = float(np.float64(np.float32(grad_scale))) * math.sqrt(sumsq) if sumsq == sumsq and sumsq >= 0 else float("nan")
    finite = math.isfinite(norm)
    clip = min(1.0, max_norm / (norm + 1e-6)) if (max_norm > 0 and finite) else 1.0
    return sumsq, norm, clip, finite


def adam_tail_host(p, g, m, v, ema, lr, betas, eps, step, grad_scale=1.0, clip=1.0, omd=0.0):
    """One tail step on the host -> (p, m, v, ema): Adam in fp64 on gi = (g * grad_scale) * clip (torch.optim.Adam, no amsgrad, no
    weight decay), then, if `ema` is given, s <- s - omd * (s - p_new) in fp32 on the fp32 rounding of p_new: three separately rounded
    operations, upstream's `s_param.sub_(one_minus_decay * (s_param - param))`."""
    b1, b2 = betas
    p, g, m, v = (torch.as_tensor(t).detach().cpu().to(torch.float64) for t in (p, g, m, v))
    gi = g * grad_scale * clip
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (torch.sqrt(v) / (bc2 ** 0.5) + eps))
    if ema is not None:
        s = np.asarray(ema.detach().cpu() if torch.is_tensor(ema) else ema, dtype=np.float32)
        pn = p.to(torch.float32).numpy()
        d = (s - pn).astype(np.float32)
        t = (np.float32(omd) * d).astype(np.float32)
        ema = torch.from_numpy((s - t).astype(np.float32))
    return p, m, v, ema
