"""Patient scoring with surface metrics: host (scipy) path against the device path, next to the prediction it scores.

For the two phantom sizes of tests/test_surface_gpu.py (10x192x192 and 40x256x256, 4 classes) and the metric lists
("Dice", "HD") and ("Dice", "HD", "ASD") this times, per patient,
  host    what `runningMySegmentationScore.update` did for device volumes before the device path existed: voxel counts from the
          confusion-matrix kernel, both label volumes copied to the host, scipy erosion + distance transform per class / direction / slice
  device  `update` as it is now (ops.surface_stats, one readback of the small tables)
  predict `tester.predict_volume` on a volume of the same size (FTN + STN, n_iter = 2, eval BatchNorm, arg-max)
each as the median over repeated calls after a warm-up, with a device synchronise on both sides of every timed call, checks that
both paths return the same row, and writes profiles/surface_metrics.json.

    python tools/bench_surface.py [--out profiles/surface_metrics.json] [--host-reps 3] [--device-reps 30]
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, metrics  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.metrics import runningMySegmentationScore  # noqa: E402

SPACING = (10.0, 1.25, 1.25)
N_CLASS = 4


def phantom(d, h, w, jitter, seed):
    rng = np.random.RandomState(seed)
    vol = np.zeros((d, h, w), dtype=np.int64)
    y, x = np.mgrid[0:h, 0:w]
    for z in range(d):
        cy, cx = h / 2 + rng.uniform(-jitter, jitter), w / 2 + rng.uniform(-jitter, jitter)
        r = np.hypot(y - cy, (x - cx) / 1.2)
        s = 1 - 0.5 * abs(z - d / 2) / d
        for lab, frac in ((1, 0.30), (2, 0.22), (3, 0.15)):
            vol[z][r < frac * h * s] = lab
    return vol


def host_update(ms, preds_d, gts_d, spacing):
    """The row as `update` computed it for device volumes with the surface metrics on the host."""
    pc, gc, ic = ms._counts(preds_d, gts_d)
    p_h, g_h = preds_d.detach().cpu().numpy(), gts_d.detach().cpu().numpy()
    row = ["p"]
    for c in range(1, ms.n_classes):
        for m in ms.metrics:
            if m == "Dice":
                v1, v2 = int(pc[c]), int(gc[c])
                row.append(2.0 * int(ic[c]) / float(v1 + v2) if v1 + v2 else 0.0)
            elif m == "HD":
                row.append(float(metrics.hd_2D_stack(p_h == c, g_h == c, pixelspacing=spacing[:2], connectivity=2)))
            else:
                row.append(float(metrics.asd(p_h == c, g_h == c, voxelspacing=spacing, connectivity=2)))
    return row


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics.json"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device-reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=N_CLASS, use_gpu=True)
    solver.eval()
    rows = []
    for d, h, w in ((10, 192, 192), (40, 256, 256)):
        pr = torch.from_numpy(phantom(d, h, w, 6, 1).astype(np.uint8)).cuda()
        gt = torch.from_numpy(phantom(d, h, w, 3, 0)).cuda()
        image = torch.rand(d, 1, h, w, generator=torch.Generator().manual_seed(5)).cuda()
        _, t_pred, _, _ = timed(lambda: predict_volume(solver, image, n_iter=2, chunk=10), args.device_reps, 3)
        for mlist in (("Dice", "HD"), ("Dice", "HD", "ASD")):
            ms = runningMySegmentationScore(N_CLASS, metrics_list=list(mlist))
            before = _ffi.lib.ctl_launch_count()
            ms.update("p", pr, gt, voxel_spacing=SPACING)
            launches = int(_ffi.lib.ctl_launch_count() - before)
            row_h, t_host, h_lo, h_hi = timed(lambda: host_update(ms, pr, gt, SPACING), args.host_reps, 1)
            row_d, t_dev, d_lo, d_hi = timed(lambda: ms.update("p", pr, gt, voxel_spacing=SPACING), args.device_reps, 3)
            diff = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(row_d[1:], row_h[1:]))
            assert diff <= 1e-12, (row_d, row_h)
            rec = {"volume": [d, h, w], "n_classes": N_CLASS, "voxel_spacing": list(SPACING), "metrics": list(mlist),
                   "host_ms": t_host * 1e3, "host_ms_min_max": [h_lo * 1e3, h_hi * 1e3], "host_reps": args.host_reps,
                   "device_ms": t_dev * 1e3, "device_ms_min_max": [d_lo * 1e3, d_hi * 1e3], "device_reps": args.device_reps,
                   "host_over_device": t_host / t_dev, "predict_volume_ms": t_pred * 1e3,
                   "scoring_over_predict_host": t_host / t_pred, "scoring_over_predict_device": t_dev / t_pred,
                   "kernel_launches_per_update": launches, "max_relative_row_difference": diff}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    out = {"what": "runningMySegmentationScore.update per patient: surface metrics on the host (scipy, after copying both label volumes) vs on "
                   "the device (ops.surface_stats); medians of wall time around device synchronises; predict_volume = FTN + STN n_iter=2 on "
                   "a volume of the same size",
           "launches": "2 (confusion matrices) + 4 per 'HD' (per-slice 2-D form) + 5 per 'ASD' (3-D form), independent of slices and classes",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip, "torch": torch.__version__, "host": platform.node(),
           "host_cpus_usable": len(os.sched_getaffinity(0)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
