"""Image-similarity losses (csrc/ctl_recon.hip) at 16 x 1 x 256 x 256 and 16 x 1 x 192 x 192: a random image and a prediction that mostly agrees.

Device time between HIP events, warm, median over repeated batches of `--inner` calls divided by the batch, eager (the calls as issued
from Python, launch gaps included) and as the replay of one captured graph, of forward + backward (ops.recon_loss_fwd / _bwd with a device
gout) of
  each kind alone and {'mse': 1, 'lncc': 0.1} fused (win = 9), next to `scaled_mse` alone (ops.mse_fwd / mse_bwd, today's reconstruction term)
and next to the ATen composition of the same results on the same tensors (conv2d with an all-ones filter for 'lncc', cosine_similarity
for 'ncc', autograd for the gradient), timed the same way.  `bytes`: what forward + backward must move (x and t read by each, dx written
once: 5 tensors) and what the launches of the set move -- for 'lncc' the tiled passes also write and read the three fp64 coefficient maps
(24 bytes per pixel each way) -- with the fraction of the achievable HBM rate (6.3 TB/s) the graph time implies.  Then the wall time of an
eager `cooperative_step` at 16 x 256 x 256 with the default reconstruction loss and with the fused pair.  Nothing is asserted about the
times.  Writes profiles/recon_loss.json.

    python tools/bench_recon.py [--out profiles/recon_loss.json] [--reps 20] [--inner 20] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cc import device_ms  # noqa: E402
from bench_restore import captured  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import ops, recon  # noqa: E402

B, C, WIN, BETA = 16, 1, 9, 1.0 / 9
SIZES = [(256, 256), (192, 192)]
HBM_ACHIEVABLE = 6.3e12
PAIR = {"mse": 1.0, "lncc": 0.1}
DROP_MSE = {"loss_name": "mse", "mask_type": "dropout", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
DROP_CE = {"loss_name": "ce", "mask_type": "dropout", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}


def per_call(fn, reps, inner):
    med, lo, hi = device_ms(lambda: [fn() for _ in range(inner)], reps)
    return {"ms": med / inner, "ms_min_max": [lo / inner, hi / inner]}


def both(fn, reps, inner):
    rec = {"eager": per_call(fn, reps, inner)}
    graph = captured(fn)
    rec["graph"] = per_call(graph.replay, reps, inner)
    del graph
    return rec


def aten_total(x, t, kinds, ones):
    """the same results as ATen ops (upstream's operations, custom_loss.py:310-318, :514-571, :574-661)"""
    total = 0.0
    b = x.shape[0]
    for name, weight in kinds.items():
        if name == "mse":
            l = F.mse_loss(x, t)
        elif name == "l1":
            l = F.l1_loss(x, t)
        elif name == "smooth l1":
            n = torch.abs(x - t)
            l = torch.where(n < BETA, 0.5 * n ** 2 / BETA, n - 0.5 * BETA).mean()
        elif name == "ncc":
            xm, tm = x - x.mean((2, 3), keepdim=True), t - t.mean((2, 3), keepdim=True)
            l = 1 - F.cosine_similarity(xm.reshape(b, -1), tm.reshape(b, -1), dim=1, eps=1e-6).sum() / b
        else:
            conv = lambda v: F.conv2d(v, ones, padding=WIN // 2)      # noqa: E731
            I_sum, J_sum, I2_sum, J2_sum, IJ_sum = conv(t), conv(x), conv(t * t), conv(x * x), conv(x * t)
            A = float(WIN * WIN)
            uI, uJ = I_sum / A, J_sum / A
            cross = IJ_sum - uJ * I_sum - uI * J_sum + uI * uJ * A
            I_var = I2_sum - 2 * uI * I_sum + uI * uI * A
            J_var = J2_sum - 2 * uJ * J_sum + uJ * uJ * A
            l = 1 - torch.mean(cross / (torch.sqrt(I_var) * torch.sqrt(J_var) + 1e-6))
        total = total + weight * l
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_loss.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon.py measures on the GPU: no device found")
    gout = torch.tensor(0.7, device="cuda")
    ones = torch.ones(C, C, WIN, WIN, device="cuda")
    sets = [{n: 1.0} for n in ops.RECON_KINDS] + [PAIR]
    sizes = {}
    for h, w in SIZES:
        g = torch.Generator().manual_seed(0)
        t = torch.randn(B, h, w, C, generator=g).permute(0, 3, 1, 2)
        x = t + 0.3 * torch.randn(B, h, w, C, generator=g).permute(0, 3, 1, 2)
        xd, td = x.cuda(), t.cuda()
        tensor = B * C * h * w * 4
        maps = B * h * w * 24

        def scaled_mse():
            return ops.mse_fwd(xd, td, 0.5), ops.mse_bwd(xd, td, gout, 0.5)

        rec = {"scaled_mse": both(scaled_mse, args.reps, args.inner)}
        for kinds in sets:
            def fused():
                loss, _, ws = ops.recon_loss_fwd(xd, td, kinds, beta=BETA, win=WIN)
                return loss, ops.recon_loss_bwd(xd, td, kinds, gout, ws, beta=BETA, win=WIN)

            def aten():
                xr = xd.detach().requires_grad_(True)
                loss = aten_total(xr, td, kinds, ones)
                return loss, torch.autograd.grad(loss, [xr], gout)[0]

            loss, grad = fused()
            ref = recon.similarity_and_grad(x, t, kinds, beta=BETA, win=WIN, gout=float(np.float32(0.7)))
            al, ag = aten()
            stream, lncc = any(n != "lncc" for n in kinds), "lncc" in kinds
            moved = tensor * (2 * int(stream) + 2 * int(lncc) + 3) + 2 * maps * int(lncc)
            e = {"loss": float(ref.loss), "loss_error_abs": abs(float(loss) - float(ref.loss)), "grad_abs_max": float(ref.grad.abs().max()),
                 "grad_error_abs_max": float((grad.cpu().double() - ref.grad).abs().max()), "flagged_windows": ref.flagged,
                 "aten_loss_error_abs": abs(float(al) - float(ref.loss)), "aten_grad_error_abs_max": float((ag.cpu().double() - ref.grad).abs().max()),
                 "fused": both(fused, args.reps, args.inner), "aten": both(aten, args.reps, args.inner)}
            e["aten_over_fused_graph"] = e["aten"]["graph"]["ms"] / e["fused"]["graph"]["ms"]
            e["aten_over_fused_eager"] = e["aten"]["eager"]["ms"] / e["fused"]["eager"]["ms"]
            e["fused_over_scaled_mse_graph"] = e["fused"]["graph"]["ms"] / rec["scaled_mse"]["graph"]["ms"]
            ms = e["fused"]["graph"]["ms"]
            e["bytes"] = {"must_move": 5 * tensor, "launches_move": moved, "must_move_fraction_of_6.3TBs": 5 * tensor / (ms * 1e-3) / HBM_ACHIEVABLE,
                          "launches_move_fraction_of_6.3TBs": moved / (ms * 1e-3) / HBM_ACHIEVABLE}
            rec["+".join(kinds)] = e
        sizes[f"{B}x{C}x{h}x{w}"] = rec
        print(json.dumps({f"{B}x{C}x{h}x{w}": rec}), flush=True)

    from oracle import ref_cpu as O
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    dev = lambda v: v.cuda().contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.cuda()      # noqa: E731
    h, w = SIZES[0]
    batch = tuple(dev(v) for v in O.synthetic_batch(B, h, w, seed=5))
    steps = {}
    for label, kw in (("default", {}), ("mse+lncc", dict(recon_loss_type={"mse": 1, "lncc": 0.1}, recon_loss_params={"win": WIN}))):
        torch.manual_seed(0)
        s = AdvancedTripletReconSegmentationModel(use_gpu=True, **kw)
        for _ in range(5):
            s.cooperative_step(*batch, DROP_MSE, DROP_CE)
        times = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.cooperative_step(*batch, DROP_MSE, DROP_CE)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        steps[label] = {"ms": float(np.median(times)), "ms_min_max": [min(times), max(times)]}
        print(json.dumps({label: steps[label]}), flush=True)
        del s
    res = {"what": f"image-similarity losses on {B}x{C}xHxW fp32 NHWC images: device time between HIP events per forward + backward (median of "
                   f"{args.reps} batches of {args.inner} calls, warm), eager and as the replay of one captured graph; fused = the kernels of "
                   "ctl_recon.hip, aten = the same results as ATen ops with autograd on the same tensors, scaled_mse = ctl_mse_fwd / _bwd; errors of "
                   "both against the fp64 host statement (recon.py), gout = 0.7; bytes = what forward + backward must move / what the launches of "
                   f"the set move (the fp64 maps of 'lncc' included) as a fraction of 6.3 TB/s at the fused graph time; eager_step_ms = wall time of "
                   f"an eager cooperative_step at {B}x{h}x{w} (synchronised, median of {args.steps})",
           "thresholds": "none",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "sizes": sizes, "eager_step_ms": steps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
