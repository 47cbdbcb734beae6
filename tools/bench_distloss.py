"""Distance-map losses (csrc/ctl_dist.hip, csrc/ctl_loss.hip) at 16 x 4 x 256 x 256 and 16 x 4 x 192 x 192: labels of smooth blobs, logits that
mostly agree with them.

Device time between HIP events, warm, median over repeated batches of `--inner` calls divided by the batch, eager (the calls as issued
from Python, launch gaps included) and as the replay of one captured graph, of
  class_fields       each training form ('signed', 'squared') of an int64 label map
  confident_label    the thresholding of the logits
  each loss          forward + backward (ops.dist_loss_fwd, ops.dist_loss_bwd with a device gout) with the fields given, and with every field
                     it needs computed in the same call ('hausdorff dt': label fields, confident label, prediction fields)
next to the same loss composed the usual way on the same machine: scipy.ndimage.distance_transform_edt on the host for the maps (the
labels, and for 'hausdorff dt' the thresholded prediction, copied from the device and the maps back to it) plus ATen ops and autograd for
the value and the gradient; host wall time around a synchronise.  Then the wall time of an eager `cooperative_step` with seg_loss_type
'dice', {'dice': 1, 'boundary': 0.01} and {'dice': 1, 'hausdorff dt': 1e-3}.  `field_bytes`: what ctl_class_fields must move (labels
in, fields out) and what it moves with its two uint16 row maps written and read once, and the HBM rates the graph time implies.  Nothing is
asserted about the times.  Writes profiles/dist_loss.json.

    python tools/bench_distloss.py [--out profiles/dist_loss.json] [--reps 20] [--inner 20] [--host-reps 3] [--steps 20]
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

B, C = 16, 4
SIZES = [(256, 256), (192, 192)]
NAMES = ["boundary", "hausdorff dt"]
IMG_CFG = {"loss_name": "mse", "mask_type": "channel", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
SEG_CFG = {"loss_name": "ce", "mask_type": "spatial", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}


def per_call(fn, reps, inner):
    med, lo, hi = device_ms(lambda: [fn() for _ in range(inner)], reps)
    return {"ms": med / inner, "ms_min_max": [lo / inner, hi / inner]}


def both(fn, reps, inner):
    rec = {"eager": per_call(fn, reps, inner)}
    graph = captured(fn)
    rec["graph"] = per_call(graph.replay, reps, inner)
    del graph
    return rec


def host_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(times)), "ms_min_max": [min(times), max(times)]}


def scipy_fields(label_dev, signed):
    """the maps of a device label map [B,H,W] the usual way: copy to the host, scipy per slice and class, copy back (fp32 NCHW)"""
    f = losses.class_fields_host(label_dev.cpu(), C)
    f = losses.signed_from_fields(f, label_dev.cpu()) if signed else f * f
    return f.float().to(label_dev.device)


def scipy_aten(xd, yd, name, gout):
    xr = xd.detach().requires_grad_(True)
    p = torch.softmax(xr, 1)
    if name == "boundary":
        loss = (p * scipy_fields(yd, True))[:, 1:].mean()
    else:
        q = torch.where((p > 0.5).any(1), (p > 0.5).float().argmax(1), torch.full((), 255, device=xd.device))
        d = scipy_fields(yd, False) + scipy_fields(q, False)
        t = torch.nn.functional.one_hot(yd, C).permute(0, 3, 1, 2).float()
        loss = (((p - t) ** 2) * d)[:, 1:].mean()
    return loss, torch.autograd.grad(loss, [xr], gout)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_loss.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distloss.py measures on the GPU: no device found")
    from oracle import ref_cpu as O
    gout = torch.tensor(0.7, device="cuda")
    sizes = {}
    for h, w in SIZES:
        g = torch.Generator().manual_seed(0)
        y = O.synthetic_batch(B, h, w, seed=0)[1].long()
        x = (torch.randn(B, h, w, C, generator=g) + 4.0 * torch.nn.functional.one_hot(y.roll(3, 2), C)).permute(0, 3, 1, 2)
        xd, yd = x.cuda(), y.cuda()
        rec = {}
        for form in ("signed", "squared"):
            rec["class_fields " + form] = both(lambda: ops.class_fields(yd, C, form), args.reps, args.inner)
        rec["confident_label"] = both(lambda: ops.confident_label(xd), args.reps, args.inner)
        must = B * h * w * 8 + B * C * h * w * 4
        moved = must + 2 * B * C * h * w * 2 * 2 + (C - 1) * B * h * w * 8       # row maps written and read; the labels once per class in the row pass
        ms = rec["class_fields signed"]["graph"]["ms"]
        rec["field_bytes"] = {"must_move": must, "with_row_maps": moved, "must_move_GBps": must / ms / 1e6, "with_row_maps_GBps": moved / ms / 1e6}
        for name in NAMES:
            fa = ops.class_fields(yd, C, ops.DIST_LOSS_FORM[name])
            fb = ops.class_fields(ops.confident_label(xd), C, "squared") if name == "hausdorff dt" else None

            def given():
                return ops.dist_loss_fwd(xd, yd, name, fa, fb), ops.dist_loss_bwd(xd, yd, name, gout, fa, fb)

            def whole():
                a = ops.class_fields(yd, C, ops.DIST_LOSS_FORM[name])
                b = ops.class_fields(ops.confident_label(xd), C, "squared") if name == "hausdorff dt" else None
                return ops.dist_loss_fwd(xd, yd, name, a, b), ops.dist_loss_bwd(xd, yd, name, gout, a, b)

            loss, grad = whole()
            ref_loss, ref_grad = losses.loss_and_grad(x, y, name, gout=float(np.float32(0.7)),
                                                      pred_fields=losses.class_fields_host(ops.confident_label(xd).cpu(), C))
            r = {"loss_error_abs": abs(float(loss) - float(ref_loss)), "grad_error_abs_max": float((grad.cpu().double() - ref_grad).abs().max()),
                 "loss": float(ref_loss), "grad_abs_max": float(ref_grad.abs().max()),
                 "fields_given": both(given, args.reps, args.inner), "fields_computed": both(whole, args.reps, args.inner),
                 "scipy_aten": host_ms(lambda: scipy_aten(xd, yd, name, gout), args.host_reps)}
            r["scipy_aten_over_graph"] = r["scipy_aten"]["ms"] / r["fields_computed"]["graph"]["ms"]
            rec[name] = r
        sizes[f"{B}x{C}x{h}x{w}"] = rec
        print(json.dumps({f"{B}x{C}x{h}x{w}": rec}), flush=True)

    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    dev = lambda t: t.cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.cuda()      # noqa: E731
    h, w = SIZES[0]
    batch = tuple(dev(t) for t in O.synthetic_batch(B, h, w, seed=0))
    steps = {}
    for label, spec in (("dice", "dice"), ("dice + 0.01 boundary", {"dice": 1, "boundary": 0.01}),
                        ("dice + 0.001 hausdorff dt", {"dice": 1, "hausdorff dt": 1e-3})):
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
        steps[label] = {"ms": float(np.median(times)), "ms_min_max": [min(times), max(times)]}
        print(json.dumps({"cooperative_step " + label: steps[label]}), flush=True)
        del s
    res = {"what": f"distance-map losses on {B}x{C}xHxW fp32 NHWC logits and int64 labels: device time between HIP events per call (median of "
                   f"{args.reps} batches of {args.inner} calls, warm), eager and as the replay of one captured graph; fields_given = forward + "
                   "backward of the loss kernels alone, fields_computed = with every field the loss reads computed in the same call; scipy_aten "
                   f"= the same loss from scipy distance transforms on the host plus ATen ops and autograd (host wall time, median of {args.host_reps}); "
                   "errors against the fp64 host statement (losses.py) with the device's confident label, gout = 0.7; field_bytes = bytes "
                   "ctl_class_fields must move / moves with its row maps, and the rates the 'signed' graph time implies; cooperative_step = eager "
                   f"step wall time at {B}x{h}x{w} (channel / spatial masks, synchronised, median of {args.steps}) per seg_loss_type",
           "thresholds": "none",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "sizes": sizes, "cooperative_step_ms": steps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
