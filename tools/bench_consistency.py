"""Consistency losses (csrc/ctl_consist.hip) at 16 x 4 x 256 x 256 and 16 x 4 x 192 x 192: random logits, a reference that mostly agrees.

Device time between HIP events, warm, median over repeated batches of `--inner` calls divided by the batch, eager (the calls as issued
from Python, launch gaps included) and as the replay of one captured graph, of forward + backward (ops.consistency_fwd / _bwd with a device
gout; with scales, autograd through calc_segmentation_consistency) of
  each kind alone, ['kl', 'contour'] (the default), all six names together, and the default at scales = [0, 1, 2]
next to the ATen composition of upstream's operations on the same tensors (softmax / log_softmax, a one-channel conv2d per class and filter
for 'contour', avg_pool2d, autograd for the gradient), timed the same way.  `bytes`: what forward + backward must move (x and r read by
each, dlogit written once: 5 tensors) and what the launches of the set move (a tensor more per extra pass, two more where the contour
launch adds into dlogit), with the HBM rates the graph time implies.  Then the wall time of an eager `consistency_training` call
(forward, backward, optimizer step of the two networks it trains) next to `standard_training` on the same batch.  Nothing is asserted
about the times.  Writes profiles/consistency_loss.json.

    python tools/bench_consistency.py [--out profiles/consistency_loss.json] [--reps 20] [--inner 20] [--steps 20]
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
from cooperative_training_and_latent_space_data_augmentation_amd import consistency as K, ops  # noqa: E402

B, C = 16, 4
SIZES = [(256, 256), (192, 192)]
NAMES = list(ops.CONSISTENCY_KINDS)
CW = [0.5, 1.0, 2.5, 1.5]
SX = [[1.0, 0.0, -1.0], [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]]
SY = [[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]]


def per_call(fn, reps, inner):
    med, lo, hi = device_ms(lambda: [fn() for _ in range(inner)], reps)
    return {"ms": med / inner, "ms_min_max": [lo / inner, hi / inner]}


def both(fn, reps, inner):
    rec = {"eager": per_call(fn, reps, inner)}
    graph = captured(fn)
    rec["graph"] = per_call(graph.replay, reps, inner)
    del graph
    return rec


def aten_total(x, r, names, weights, scales, sx, sy, cw):
    """upstream's operations (custom_loss.py:892-973 and what it calls) as ATen ops, without its host reads"""
    total = 0.0
    c = x.shape[1]
    for s in scales:
        xs, rs = (F.avg_pool2d(x, 2 ** s), F.avg_pool2d(r, 2 ** s)) if s else (x, r)
        n, _, h, w = xs.shape
        for name, weight in zip(names, weights):
            if name == "kl":
                p, logp = F.softmax(rs, 1), F.log_softmax(rs, 1)
                l = torch.mean(torch.sum(p * logp, 1, keepdim=True) - torch.sum(p * F.log_softmax(xs, 1), 1, keepdim=True))
            elif name in ("ce", "weighted ce"):
                t = F.softmax(rs, 1) * F.log_softmax(xs, 1)
                l = -(t.sum() if name == "ce" else (t * cw.view(1, c, 1, 1)).sum()) / (n * h * w)
            elif name == "mse":
                l = F.mse_loss(F.softmax(xs, 1), F.softmax(rs, 1), reduction="sum") / (n * h * w)
            elif name == "Dice":
                q, p = F.softmax(xs, 1).view(n, c, -1), F.softmax(rs, 1).view(n, c, -1)
                l = 1.0 - torch.sum(2.0 * (torch.sum(q * p, 2) + 0.01) / (torch.sum(q, 2) + torch.sum(p, 2) + 0.01)) / (n * c)
            else:
                q, p = F.softmax(xs, 1), F.softmax(rs, 1)
                l = 0.0
                for k in range(1, c):
                    a, t = q[:, [k]], p[:, [k]]
                    l = l + 0.5 * (F.mse_loss(F.conv2d(a, sx, padding=1), F.conv2d(t, sx, padding=1)) +
                                   F.mse_loss(F.conv2d(a, sy, padding=1), F.conv2d(t, sy, padding=1)))
                l = l / (c - 1)
            total = total + 2 ** s * weight * l
    return total / len(scales)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_loss.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency.py measures on the GPU: no device found")
    gout = torch.tensor(0.7, device="cuda")
    sx, sy = torch.tensor(SX, device="cuda").view(1, 1, 3, 3), torch.tensor(SY, device="cuda").view(1, 1, 3, 3)
    cwn = torch.tensor(CW, device="cuda") / sum(CW) * C
    sets = [([n], [1.0], [0]) for n in NAMES] + [(["kl", "contour"], [1.0, 0.5], [0]), (NAMES, [1.0, 0.5, 0.3, 2.0, 0.7, 1.5], [0]),
                                                (["kl", "contour"], [1.0, 0.5], [0, 1, 2])]
    sizes = {}
    for h, w in SIZES:
        g = torch.Generator().manual_seed(0)
        r = (torch.randn(B, h, w, C, generator=g) * 3.0).permute(0, 3, 1, 2)
        x = r + torch.randn(B, h, w, C, generator=g).permute(0, 3, 1, 2)
        xd, rd = x.cuda(), r.cuda()
        tensor = B * C * h * w * 4
        rec = {}
        for names, weights, scales in sets:
            kinds = dict(zip(names, weights))

            def fused():
                if scales == [0]:
                    loss, _, ws = ops.consistency_fwd(xd, rd, kinds, CW)
                    return loss, ops.consistency_bwd(xd, rd, kinds, gout, ws, CW)
                xr = xd.detach().requires_grad_(True)
                loss = K.calc_segmentation_consistency(xr, rd, names, weights, CW, scales)
                return loss, torch.autograd.grad(loss, [xr], gout)[0]

            def aten():
                xr = xd.detach().requires_grad_(True)
                loss = aten_total(xr, rd, names, weights, scales, sx, sy, cwn)
                return loss, torch.autograd.grad(loss, [xr], gout)[0]

            loss, grad = fused()
            ref_loss, ref_grad = K.consistency_and_grad(x, r, names, weights, CW, scales, gout=float(np.float32(0.7)))
            al, ag = aten()
            pw, ct = any(n != "contour" for n in names), "contour" in names
            moved = tensor * (2 * int(pw) + 2 * int(ct) + 3 * int(pw) + (4 if pw and ct else 3 if ct else 0))
            e = {"loss": float(ref_loss), "loss_error_abs": abs(float(loss) - float(ref_loss)), "grad_abs_max": float(ref_grad.abs().max()),
                 "grad_error_abs_max": float((grad.cpu().double() - ref_grad).abs().max()),
                 "aten_loss_error_abs": abs(float(al) - float(ref_loss)), "aten_grad_error_abs_max": float((ag.cpu().double() - ref_grad).abs().max()),
                 "fused": both(fused, args.reps, args.inner), "aten": both(aten, args.reps, args.inner)}
            e["aten_over_fused_graph"] = e["aten"]["graph"]["ms"] / e["fused"]["graph"]["ms"]
            e["aten_over_fused_eager"] = e["aten"]["eager"]["ms"] / e["fused"]["eager"]["ms"]
            if scales == [0]:
                ms = e["fused"]["graph"]["ms"]
                e["bytes"] = {"must_move": 5 * tensor, "launches_move": moved, "must_move_GBps": 5 * tensor / ms / 1e6, "launches_move_GBps": moved / ms / 1e6}
            rec["+".join(names) + ("" if scales == [0] else " scales=" + str(scales))] = e
        sizes[f"{B}x{C}x{h}x{w}"] = rec
        print(json.dumps({f"{B}x{C}x{h}x{w}": rec}), flush=True)

    from oracle import ref_cpu as O
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    dev = lambda t: t.cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.cuda()      # noqa: E731
    h, w = SIZES[0]
    clean, label, noisy = (dev(t) for t in O.synthetic_batch(B, h, w, seed=0))
    torch.manual_seed(0)
    s = AdvancedTripletReconSegmentationModel(use_gpu=True)
    s.train()

    def consistency_step():
        s.zero_grad()
        s.consistency_training(clean, noisy, target="stn", divergence_types=("kl", "contour"), divergence_weights=(1.0, 0.5)).backward()
        s.optimize_params("image_encoder")
        s.optimize_params("segmentation_decoder")

    def standard_step():
        s.zero_grad()
        sum(s.standard_training(clean, label, noisy)).backward()
        s.optimize_all_params()

    steps = {}
    for label_, fn in (("consistency_training kl+contour target=stn", consistency_step), ("standard_training", standard_step)):
        for _ in range(5):
            fn()
        times = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        steps[label_] = {"ms": float(np.median(times)), "ms_min_max": [min(times), max(times)]}
        print(json.dumps({label_: steps[label_]}), flush=True)
    res = {"what": f"consistency losses on {B}x{C}xHxW fp32 NHWC logits: device time between HIP events per forward + backward (median of {args.reps} "
                   f"batches of {args.inner} calls, warm), eager and as the replay of one captured graph; fused = the kernels of ctl_consist.hip, aten = "
                   "upstream's operations as ATen ops with autograd on the same tensors; errors of both against the fp64 host statement "
                   "(consistency.py), gout = 0.7; bytes = what forward + backward must move / what the launches of the set move, and the rates "
                   f"the fused graph time implies; eager_step_ms = wall time at {B}x{h}x{w} of forward + backward + optimizer step "
                   f"(synchronised, median of {args.steps})",
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
