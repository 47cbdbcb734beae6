#!/usr/bin/env python3
"""Golden vectors of the optimizer tail's host objects, produced by the REAL reference classes on the CPU
(medseg/models/model_util.py: ExponentialMovingAverage :21-101, lr_poly :589-590, get_scheduler :621-671).  Build container only:
    python tools/gen_golden_optim.py  ->  tests/golden/optim_cases.pt
  ema    per (dtype, use_num_updates): the start parameters, the 30 parameter sets fed to update(), the shadows after 1, 3 and 30 updates
  sched  per policy: base lr, get_scheduler's keywords, the metric series (plateau policies) and the lr sequence
         [at construction, after step 1, ...] read from a real torch.optim.Adam
  poly   (base_lr, iter, max_iter, power, value) rows of lr_poly
Only tensors and numbers are written."""
import os
import sys
import warnings
from unittest.mock import MagicMock

for _m in ["numpy.lib.function_base", "SimpleITK", "medpy", "medpy.metric", "medpy.metric.binary", "IPython",
           "IPython.display", "skimage", "skimage.transform", "seaborn"]:
    sys.modules[_m] = MagicMock()
sys.path.insert(0, os.environ.get("CTL_REFERENCE", "/root/reference"))

import torch  # noqa: E402

import medseg.models.model_util as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "optim_cases.pt")
SHAPES = [(3, 5), (7,), (1,)]
DECAY = 0.999
BASE_LR = 1e-4


def ema_cases():
    cases = []
    for dtype in (torch.float32, torch.float64):
        for use_num_updates in (True, False):
            g = torch.Generator().manual_seed(5)
            start = [torch.randn(s, generator=g, dtype=dtype) for s in SHAPES]
            params = [torch.nn.Parameter(t.clone()) for t in start]
            ema = ref.ExponentialMovingAverage(params, DECAY if use_num_updates else 0.9, use_num_updates=use_num_updates)
            feed, shadows = [], {}
            for n in range(1, 31):
                step = [0.05 * torch.randn(s, generator=g, dtype=dtype) for s in SHAPES]
                with torch.no_grad():
                    for p, d in zip(params, step):
                        p.add_(d)
                feed.append([p.detach().clone() for p in params])
                ema.update(params)
                if n in (1, 3, 30):
                    shadows[n] = [s.detach().clone() for s in ema.shadow_params]
            cases.append({"dtype": str(dtype).replace("torch.", ""), "use_num_updates": use_num_updates, "decay": ema.decay,
                          "start": start, "feed": feed, "shadows": shadows})
    return cases


def stalling_series(n):
    """falls, stalls for longer than the patience, falls a little, stalls again: both plateau policies cut the rate more than once"""
    out, v = [], 2.0
    for i in range(n):
        if i < 6 or 20 <= i < 23:
            v *= 0.8
        out.append(v + (0.001 if i % 2 else 0.0))
    return out


def sched_cases():
    specs = [("lambda", dict(epoch_count=0, niter=3, niter_decay=4), 8), ("step", dict(lr_decay_iters=5), 23),
             ("step", dict(lr_decay_iters=1), 12), ("step2", dict(lr_decay_iters=3), 14), ("plateau", {}, 40), ("plateau2", {}, 40),
             ("step_warmstart", {}, 210), ("step_warmstart2", {}, 110)]
    cases = []
    for policy, kw, n in specs:
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=BASE_LR)
        sch = ref.get_scheduler(opt, policy, **kw)
        metrics = stalling_series(n) if policy.startswith("plateau") else None
        lrs = [opt.param_groups[0]["lr"]]
        for i in range(n):
            opt.step()
            if metrics is None:
                sch.step()
            else:
                sch.step(metrics[i])
            lrs.append(opt.param_groups[0]["lr"])
        cases.append({"policy": policy, "kwargs": kw, "base_lr": BASE_LR, "metrics": metrics, "lrs": [float(v) for v in lrs]})
    return cases


def poly_cases():
    return [(b, i, m, p, float(ref.lr_poly(b, i, m, p))) for b in (1e-4, 2.5e-3) for i, m in ((0, 100), (1, 100), (37, 100), (99, 100), (500, 1200))
            for p in (0.9, 0.985)]


def main():
    warnings.simplefilter("ignore")
    sys.stdout, keep = open(os.devnull, "w"), sys.stdout      # (get_scheduler prints its policy)
    try:
        data = {"ema": ema_cases(), "sched": sched_cases(), "poly": poly_cases()}
    finally:
        sys.stdout = keep
    torch.save(data, OUT)
    print(f"wrote {OUT}: {len(data['ema'])} ema, {len(data['sched'])} schedule, {len(data['poly'])} poly cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
