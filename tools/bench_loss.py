"""Segmentation-loss kernels (csrc/ctl_loss.hip) at the flagship shape, 16 x 4 x 256 x 256 logits against a 16 x 256 x 256 label map.

Per kind ('weighted cross entropy', 'focal', 'dice', 'foreground dice'): device time of forward + backward (ops.seg_loss_fwd, then
ops.seg_loss_bwd with a device gout) between HIP events, warm, median over repeated batches of `--inner` calls, divided by the batch:
  eager   the calls as issued from Python (launch gaps included)
  graph   one forward + backward captured once, the replay timed the same way
next to `ce2d` (ops.ce2d_fwd + ops.ce2d_bwd) on the same input and to an ATen restatement of the same loss on the device (forward and
torch.autograd.grad).  Every kind's loss and gradient are compared with the fp64 host statement (losses.py) at this shape and the
errors recorded.  Then the wall time of `cooperative_step` (eager, synchronised) with seg_loss_type 'cross entropy',
'dice' and {'cross entropy': 1, 'dice': 1} (targeted channel / spatial masks).  Nothing is asserted about the times.  Writes profiles/loss_kernels.json.

    python tools/bench_loss.py [--out profiles/loss_kernels.json] [--reps 20] [--inner 20] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cc import device_ms  # noqa: E402
from bench_restore import captured  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import losses, ops  # noqa: E402

B, C, H, W = 16, 4, 256, 256
KINDS = ["weighted cross entropy", "focal", "dice", "foreground dice"]
IMG_CFG = {"loss_name": "mse", "mask_type": "channel", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
SEG_CFG = {"loss_name": "ce", "mask_type": "spatial", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
WEIGHTS = [0.5, 1.0, 2.5, 1.5]


def aten_loss(x, y, kind, w):
    """the same loss from ATen ops on the device (what the fused kernels replace)"""
    b, c = x.shape[:2]
    logp = torch.log_softmax(x, 1)
    if kind == "weighted cross entropy":
        return torch.nn.functional.nll_loss(logp, y, weight=w / w.sum() * c, reduction="sum") / y.numel()
    if kind == "focal":
        logpt = logp.gather(1, y.unsqueeze(1)).squeeze(1)
        return (-(1 - logpt.detach().exp()) ** 2 * logpt).mean()
    p = logp.exp()
    t = torch.nn.functional.one_hot(y, c).permute(0, 3, 1, 2).to(p.dtype)
    inter, union = (p * t).sum((2, 3)), p.sum((2, 3)) + t.sum((2, 3))
    if kind == "dice":
        return 1.0 - (2.0 * (inter + 0.01) / (union + 0.01)).sum() / (b * c)
    return 1.0 - ((2.0 * inter[:, 1:] + 0.01) / (union[:, 1:] + 0.01)).sum() / (b * (c - 1))


def per_call(fn, reps, inner):
    med, lo, hi = device_ms(lambda: [fn() for _ in range(inner)], reps)
    return {"ms": med / inner, "ms_min_max": [lo / inner, hi / inner]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_kernels.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU: no device found")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, H, W, C, generator=g) * 3.0).permute(0, 3, 1, 2)
    y = torch.randint(0, C, (B, H, W), generator=g)
    xd, yd = x.cuda(), y.cuda()
    gout = torch.tensor(0.7, device="cuda")
    wd = torch.tensor(WEIGHTS, device="cuda")
    rows = {}

    def ce2d():
        ops.ce2d_fwd(xd, yd)
        return ops.ce2d_bwd(xd, yd, gout)

    rows["ce2d"] = {"eager": per_call(ce2d, args.reps, args.inner)}
    graph = captured(ce2d)
    rows["ce2d"]["graph"] = per_call(graph.replay, args.reps, args.inner)
    del graph
    print(json.dumps({"ce2d": rows["ce2d"]}), flush=True)
    for kind in KINDS:
        def fused():
            loss, ws = ops.seg_loss_fwd(xd, yd, kind, WEIGHTS)
            return loss, ops.seg_loss_bwd(xd, yd, kind, gout, ws, WEIGHTS)

        def aten():
            xr = xd.detach().requires_grad_(True)
            loss = aten_loss(xr, yd, kind, wd)
            return loss, torch.autograd.grad(loss, [xr], gout)[0]

        loss, grad = fused()
        ref_loss, ref_grad = losses.loss_and_grad(x, y, kind, WEIGHTS, gout=float(np.float32(0.7)))
        rec = {"loss_error_rel": abs(float(loss) - float(ref_loss)) / max(1.0, abs(float(ref_loss))),
               "grad_error_rel_to_max": float((grad.cpu().double() - ref_grad).abs().max() / ref_grad.abs().max()),
               "eager": per_call(fused, args.reps, args.inner)}
        graph = captured(fused)
        rec["graph"] = per_call(graph.replay, args.reps, args.inner)
        del graph
        rec["aten_eager"] = per_call(aten, args.reps, args.inner)
        rec["graph_over_ce2d_graph"] = rec["graph"]["ms"] / rows["ce2d"]["graph"]["ms"]
        rec["aten_eager_over_graph"] = rec["aten_eager"]["ms"] / rec["graph"]["ms"]
        rows[kind] = rec
        print(json.dumps({kind: rec}), flush=True)

    from oracle import ref_cpu as O
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    dev = lambda t: t.cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.cuda()      # noqa: E731
    batch = tuple(dev(t) for t in O.synthetic_batch(B, H, W, seed=0))
    steps = {}
    for name, spec in (("cross entropy", "cross entropy"), ("dice", "dice"), ("cross entropy + dice", {"cross entropy": 1, "dice": 1})):
        torch.manual_seed(0)
        s = AdvancedTripletReconSegmentationModel(use_gpu=True, seg_loss_type=spec)
        for _ in range(5):
            s.cooperative_step(*batch, IMG_CFG, SEG_CFG)
        times = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.cooperative_step(*batch, IMG_CFG, SEG_CFG)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        steps[name] = {"ms": float(np.median(times)), "ms_min_max": [min(times), max(times)]}
        print(json.dumps({"cooperative_step " + name: steps[name]}), flush=True)
        del s
    res = {"what": f"forward + backward of the segmentation losses on {B}x{C}x{H}x{W} fp32 NHWC logits: device time between HIP events per call "
                   f"(median of {args.reps} batches of {args.inner} calls, warm), eager and as the replay of one captured graph; ce2d = the "
                   "cross-entropy kernels on the same input; aten_eager = the same loss and its autograd gradient from ATen ops; errors against "
                   "the fp64 host statement (losses.py), gout = 0.7; cooperative_step = eager step wall time (channel / spatial masks, synchronised, "
                   f"median of {args.steps}) per seg_loss_type",
           "thresholds": "none: a graph_over_ce2d_graph ratio above 2 is explained in DESIGN.md",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "kernels": rows, "cooperative_step_ms": steps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
