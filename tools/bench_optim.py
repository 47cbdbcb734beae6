"""The optimizer tail (csrc/ctl_optim.hip) at the five flat buffers of the shipped configuration (build_networks(1, 4, 4), real counts).

Forms, each timed eagerly (the calls as issued from Python) and as the replay of one captured graph, device time between HIP events,
warm, `--rounds` rounds in which the forms alternate (a, a again, b, c, d, e, a, ...), median / min / max over the rounds of the per-round
median over `--reps` batches of `--inner` calls:
  a        today's five ctl_adam_dev launches                                   a_repeat: the same again -- the run-to-run spread
  b        five neutral tails (lr from the record, clip = 1, no EMA)
  c        five tails with the EMA shadow
  d        control + norm + five tails with clipping, guard and EMA (the control launch stays eager in front of the replay, as in graph.py)
  e        the ATen composition of d's results: clip_grad_norm_ over the parameter views, the five ctl_adam_dev launches, upstream's
           ExponentialMovingAverage over the per-tensor views
  bytes    what each form must move (28 B / parameter for a, b; 36 for c; 40 for d: the norm reads the gradient once more) over its
           graph time, against the achievable HBM rate of 6.3 TB/s
  step     an eager cooperative_step (bs 16, 256 x 256, dropout masks) with everything on against everything off
Nothing is asserted about the times.  Writes profiles/optim_tail.json.

    python tools/bench_optim.py [--out profiles/optim_tail.json] [--rounds 5] [--reps 10] [--inner 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cc import device_ms  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import model_util, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.nets import build_networks  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.optim import FlatAdam  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-4
DROP_MSE = {"loss_name": "mse", "mask_type": "dropout", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
DROP_CE = {"loss_name": "ce", "mask_type": "dropout", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}


def captured(call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_tail.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--step-reps", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU: no device found")
    dev = torch.device("cuda")
    nets = build_networks(1, 4, 4, device=dev)
    opts = {k: FlatAdam(n, lr=LR) for k, n in nets.items()}
    counts = {k: n._pcount for k, n in nets.items()}
    total = sum(counts.values())
    g = torch.Generator(device=dev).manual_seed(1)
    for n in nets.values():
        n._flat.grad.copy_(torch.randn(n._pcount, generator=g, device=dev) * 1e-3)
    state = torch.tensor([1, 1, 10], dtype=torch.int64, device=dev)
    ctrl = ops.optim_ctrl(dev)
    emas = {k: n._flat_data.detach().clone() for k, n in nets.items()}
    work = torch.empty(ops.grad_norm_work(list(counts.values())), dtype=torch.float64, device=dev)
    lrs = [LR] * len(nets)
    views = [p for n in nets.values() for p in n.parameters()]
    aten_ema = model_util.ExponentialMovingAverage(views, 0.999)

    def adam_dev():
        for k, n in nets.items():
            ops.adam_step(n._flat_data, n._flat.grad, opts[k].exp_avg, opts[k].exp_avg_sq, LR, B1, B2, EPS, 10, 1.0, state=state)

    def tails(with_ema):
        for j, (k, n) in enumerate(nets.items()):
            ops.adam_tail(n._flat_data, n._flat.grad, opts[k].exp_avg, opts[k].exp_avg_sq, emas[k] if with_ema else None, B1, B2, EPS, 10, 1.0,
                          ctrl, j, state=state)

    def norm_and_tails():
        ops.grad_norm([n._flat.grad for n in nets.values()], 1.0, ctrl, work)
        tails(True)

    def aten():
        torch.nn.utils.clip_grad_norm_(views, 1.0)
        adam_dev()
        aten_ema.update(views)

    neutral = lambda: ops.optim_control(ctrl, lrs)                                  # noqa: E731
    full = lambda: ops.optim_control(ctrl, lrs, 1.0, True, 1e-3)                    # noqa: E731
    forms = [("a", None, adam_dev), ("a_repeat", None, adam_dev), ("b", neutral, lambda: tails(False)), ("c", full, lambda: tails(True)),
             ("d", full, norm_and_tails), ("e", None, aten)]
    bytes_per = {"a": 28, "a_repeat": 28, "b": 28, "c": 36, "d": 40, "e": None}
    graphs, errors = {}, {}
    for name, pre, body in forms:
        if pre is not None:
            pre()
        try:
            graphs[name] = captured(body)
        except Exception as exc:      # a composition that cannot be captured is reported, not hidden
            errors[name] = f"{type(exc).__name__}: {exc}"[:300]
            torch.cuda.synchronize()
    samples = {name: {"eager": [], "graph": []} for name, _, _ in forms}
    for _ in range(args.rounds):
        for name, pre, body in forms:
            def eager(pre=pre, body=body):
                for _ in range(args.inner):
                    if pre is not None:
                        pre()
                    body()
            samples[name]["eager"].append(device_ms(eager, args.reps)[0] / args.inner)
            if name in graphs:
                def replay(pre=pre, gr=graphs[name]):
                    for _ in range(args.inner):
                        if pre is not None:
                            pre()
                        gr.replay()
                samples[name]["graph"].append(device_ms(replay, args.reps)[0] / args.inner)
    out = {"device": torch.cuda.get_device_name(0), "counts": counts, "parameters": total, "rounds": args.rounds, "reps": args.reps,
           "inner": args.inner, "capture_errors": errors, "forms": {}}
    for name, _, _ in forms:
        rec = {}
        for mode, v in samples[name].items():
            if v:
                rec[mode] = {"ms": statistics.median(v), "ms_min_max": [min(v), max(v)]}
        if bytes_per[name] and "graph" in rec:
            rec["bytes"] = bytes_per[name] * total
            rec["hbm_fraction_of_6.3TBs"] = rec["bytes"] / (rec["graph"]["ms"] * 1e-3) / HBM_ACHIEVABLE
        out["forms"][name] = rec

    # an eager cooperative_step with everything on against everything off, alternating
    from oracle import ref_cpu as O
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    batch = tuple((t.to(dev).contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.to(dev)) for t in O.synthetic_batch(16, 256, 256, seed=5))
    torch.manual_seed(0)
    off = AdvancedTripletReconSegmentationModel(use_gpu=True)
    on = AdvancedTripletReconSegmentationModel(use_gpu=True, max_grad_norm=1.0, skip_nonfinite=True, use_ema=True, lr_policy="step")
    step = {"off": [], "on": []}
    for _ in range(3):
        for name, s in (("off", off), ("on", on)):
            step[name].append(device_ms(lambda s=s: s.cooperative_step(*batch, DROP_MSE, DROP_CE), args.step_reps)[0])
    out["cooperative_step_eager_bs16_256"] = {k: {"ms": statistics.median(v), "ms_min_max": [min(v), max(v)]} for k, v in step.items()}
    out["cooperative_step_eager_bs16_256"]["report_on"] = on.optim_report()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
