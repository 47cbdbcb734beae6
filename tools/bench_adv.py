"""Adversarial input augmentation (csrc/ctl_adv.hip, adversarial.py) at 16 x 1 x 256 x 256 and 16 x 1 x 192 x 192, spacing 32.

Device time between HIP events, warm, median over repeated batches of `--inner` calls divided by the batch, eager (the calls as issued
from Python, launch gaps included) and as the replay of one captured graph, of
  ops.adv_bias_fwd, ops.adv_bias_bwd (dtheta and dx), ops.adv_unit_scale on delta ('rms') and on theta ('linf'),
next to the ATen composition of the same field, adjoint and unit steps on the same tensors: two matmuls with the weight matrices, exp,
product, channel sum, two matmuls back, torch.linalg.vector_norm and a division.  `bytes`: what each call must move (fp32 tensors read
and written once; the backward's fp64 workspace is listed separately) and the fraction of the achievable HBM rate (6.3 TB/s) the graph
time implies.  Then, eager only (device time of one call, launch gaps included): one full generation with K = 1 for 'noise', 'bias' and
the chain, and one consistency_training call on the same batch for scale; and an observation, not an assertion: the supervised loss of
the fast network on x_adv against the loss on a random perturbation of the same radius (the same classes, K = 0, xi = the radius).
Nothing is asserted about the times.  Writes profiles/adv_input.json.

    python tools/bench_adv.py [--out profiles/adv_input.json] [--reps 20] [--inner 20]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cc import device_ms  # noqa: E402
from bench_restore import captured  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import adversarial as A, ops  # noqa: E402

B, C, S = 16, 1, 32
SIZES = [(256, 256), (192, 192)]
HBM_ACHIEVABLE = 6.3e12
LOG13 = math.log(1.3)


def per_call(fn, reps, inner):
    med, lo, hi = device_ms(lambda: [fn() for _ in range(inner)], reps)
    return {"ms": med / inner, "ms_min_max": [lo / inner, hi / inner]}


def both(fn, reps, inner, must_move=None):
    rec = {"eager": per_call(fn, reps, inner)}
    graph = captured(fn)
    rec["graph"] = per_call(graph.replay, reps, inner)
    del graph
    if must_move is not None:
        rec["bytes_must_move"] = must_move
        rec["fraction_of_6.3TBs_at_graph_time"] = must_move / (rec["graph"]["ms"] * 1e-3) / HBM_ACHIEVABLE
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adv_input.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adv.py measures on the GPU: no device found")
    from oracle import ref_cpu as O
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    dev = lambda v: v.cuda().contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.cuda()      # noqa: E731
    sizes = {}
    for h, w in SIZES:
        gen = torch.Generator().manual_seed(0)
        gh, gw = ops.adv_bias_grid(h, w, S)
        x = torch.rand(B, h, w, C, generator=gen).permute(0, 3, 1, 2)
        g = torch.randn(B, h, w, C, generator=gen).permute(0, 3, 1, 2) * 1e-3
        theta = (torch.rand(B, gh, gw, generator=gen) - 0.5) * 0.5
        xd, gd, td = x.cuda(), g.cuda(), theta.cuda()
        My, Mx = A.bias_weights(h, S).float().cuda(), A.bias_weights(w, S).float().cuda()
        img, grid = B * C * h * w * 4, B * gh * gw * 4
        ws = ops.lib.ctl_adv_bias_ws_bytes(B, h, w, S)

        def aten_fwd():
            return xd * torch.exp(My @ td @ Mx.T).unsqueeze(1)

        def aten_bwd():
            f = torch.exp(My @ td @ Mx.T)
            return My.T @ (f * (gd * xd).sum(1)) @ Mx, gd * f.unsqueeze(1)

        def aten_unit(v, scale, inf):
            flat = v.reshape(B, -1)
            r = torch.linalg.vector_norm(flat, float("inf") if inf else 2, dim=1, keepdim=True)
            return (scale * flat / (r if inf else r / math.sqrt(flat.shape[1]))).view_as(v)

        y = ops.adv_bias_fwd(xd, td, S)
        dtheta, dx = ops.adv_bias_bwd(gd, xd, td, S)
        yr, _ = A.bias_field_host(x, theta, S)
        dtr, dxr = A.bias_field_grad_host(g, x, theta, S)
        ady, (adt, adx) = aten_fwd(), aten_bwd()
        err = lambda a, r: float((a.cpu().double() - r).abs().max() / r.abs().max())      # noqa: E731
        rec = {"errors_rel_to_abs_max": {"x'": err(y, yr), "dtheta": err(dtheta, dtr), "dx": err(dx, dxr),
                                         "aten_x'": err(ady, yr), "aten_dtheta": err(adt, dtr), "aten_dx": err(adx, dxr)},
               "adv_bias_fwd": both(lambda: ops.adv_bias_fwd(xd, td, S), args.reps, args.inner, 2 * img + grid),
               "adv_bias_bwd": both(lambda: ops.adv_bias_bwd(gd, xd, td, S), args.reps, args.inner, 3 * img + 2 * grid),
               "adv_bias_bwd_workspace_bytes_written_and_read": 2 * ws,
               "unit_scale_delta_rms": both(lambda: ops.adv_unit_scale(gd, 0.05, "rms"), args.reps, args.inner, 3 * img),
               "unit_scale_theta_linf": both(lambda: ops.adv_unit_scale(dtheta, LOG13, "linf"), args.reps, args.inner, 3 * grid),
               "aten_bias_fwd": both(aten_fwd, args.reps, args.inner), "aten_bias_bwd": both(aten_bwd, args.reps, args.inner),
               "aten_unit_delta_rms": both(lambda: aten_unit(gd, 0.05, False), args.reps, args.inner),
               "aten_unit_theta_linf": both(lambda: aten_unit(dtheta, LOG13, True), args.reps, args.inner)}
        for k in ("bias_fwd", "bias_bwd"):
            rec[f"aten_over_hip_{k}_graph"] = rec["aten_" + k]["graph"]["ms"] / rec["adv_" + k]["graph"]["ms"]
        torch.manual_seed(0)
        s = AdvancedTripletReconSegmentationModel(use_gpu=True)
        s.train()
        clean, label, noisy = (dev(v) for v in O.synthetic_batch(B, h, w, seed=5))
        solver = {"consistency_training": per_call(lambda: s.consistency_training(clean, noisy, target="stn"), args.reps, 1)}
        losses = {}
        for name, kind in (("noise", "noise"), ("bias", "bias"), ("chain", ("bias", "noise"))):
            solver["generation_K1_" + name] = per_call(lambda: s.adversarial_example_generation(clean, label, kind, seed=1), args.reps, 1)
            radius = {"bias": {"xi": LOG13, "power_iterations": 0}, "noise": {"xi": 0.05, "power_iterations": 0}}
            rnd_params = radius if name == "chain" else radius[name]
            x_adv = s.adversarial_example_generation(clean, label, kind, seed=1)[0]
            x_rnd = s.adversarial_example_generation(clean, label, kind, seed=1, **rnd_params)[0]
            with torch.no_grad():
                sup = lambda v: float(s._seg_loss(s.fast_predict(v, disable_track_bn_stats=True)[1], label, s._label_fields(label)))      # noqa: E731
                losses[name] = {"clean": sup(clean), "adversarial_K1": sup(x_adv), "random_same_radius_K0": sup(x_rnd)}
        rec["solver_eager"] = solver
        rec["supervised_loss_untrained_network"] = losses
        del s
        sizes[f"{B}x{C}x{h}x{w}"] = rec
        print(json.dumps({f"{B}x{C}x{h}x{w}": rec}), flush=True)
    res = {"what": f"adversarial input augmentation on {B}x{C}xHxW fp32 NHWC images, control-point spacing {S}: device time between HIP events per "
                   f"call (median of {args.reps} batches of {args.inner} calls, warm), eager and as the replay of one captured graph; adv_* / "
                   "unit_scale_* = the kernels of ctl_adv.hip, aten_* = the same results as ATen ops (matmuls with the weight matrices, exp, product, "
                   "channel sum, vector_norm) on the same tensors; bytes_must_move = fp32 tensors read and written once, as a fraction of 6.3 TB/s at "
                   "the graph time; solver_eager = device time of one eager call (launch gaps included, not captured); supervised_loss = the "
                   "segmentation loss of a freshly initialised fast network on the clean batch, on x_adv (K = 1, labels given) and on a random "
                   "perturbation of the same radius (K = 0, xi = the radius): an observation",
           "thresholds": "none",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "sizes": sizes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
