"""Largest-connected-component post-processing: the device path (ops.keep_largest_components) against the host path it replaces, next to
the prediction and the scoring of the same volume.

Sizes as tools/bench_surface.py (10x192x192 and 40x256x256, 4 classes).  Inputs: the smooth phantom of that tool with 0.2 % salt noise, and
two hard cases at 256x256 per slice: a one-voxel-wide serpentine that fills every slice (one component, the longest possible path) and a
checkerboard (every voxel its own component at connectivity 1).  Per input:
  device   ops.keep_largest_components (3-D form, connectivity 1), HIP events around one call, warm, median of repeated calls
  host     what a user did before: the volume copied to the host, scipy.ndimage.label per class, keep the first largest, copied back
           (wall time between device synchronises, same box)
  launches kernels enqueued per call (the library's census; `--trace-only` under `rocprofv3 --kernel-trace --stats`, in a run of its own,
           gives the profiler's count, which `--kernel-stats` folds into the file)
and next to them tester.predict_volume and the ("Dice", "HD", "ASD") update of the same volume, and a scored patient
(TestSegmentationNetwork.evaluate, keep_results=False) with and without post_process="largest_cc".  Checks that both paths return the same
volume and that the device path is the faster one on every input, and writes profiles/cc_postprocess.json.

    python tools/bench_cc.py [--out profiles/cc_postprocess.json] [--host-reps 3] [--device-reps 30] [--kernel-stats CSV]
    rocprofv3 --kernel-trace --stats -d DIR -o cc -- python tools/bench_cc.py --trace-only
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface import phantom, timed  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.metrics import runningMySegmentationScore  # noqa: E402

SPACING = (10.0, 1.25, 1.25)
N_CLASS = 4
SALT = 0.002


def salted_phantom(d, h, w, seed):
    vol = phantom(d, h, w, 6, seed).astype(np.uint8)
    rng = np.random.RandomState(100 + seed)
    hit = rng.rand(d, h, w) < SALT
    vol[hit] = rng.randint(0, N_CLASS, size=int(hit.sum()))
    return vol


def serpentine(d, h, w):
    a = np.zeros((h, w), dtype=np.uint8)
    a[0::2] = 1
    for y in range(1, h, 2):
        a[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return np.ascontiguousarray(np.broadcast_to(a, (d, h, w)))


def checkerboard(d, h, w):
    z, y, x = np.indices((d, h, w))
    return ((z + y + x) % 2).astype(np.uint8)


def inputs():
    return [("phantom, 0.2 % salt", salted_phantom(10, 192, 192, 1)), ("phantom, 0.2 % salt", salted_phantom(40, 256, 256, 1)),
            ("serpentine", serpentine(40, 256, 256)), ("checkerboard", checkerboard(40, 256, 256))]


def host_keep_largest(vol_d):
    """The round trip the device path replaces: copy out, label every class with scipy, keep the first largest, copy back."""
    vol = vol_d.cpu().numpy()
    out = np.zeros(vol.shape, dtype=np.uint8)
    components = []
    for c in range(1, N_CLASS):
        comp, k = ndimage.label(vol == c)
        components.append(int(k))
        if k:
            out[comp == int(np.argmax(np.bincount(comp.ravel(), minlength=k + 1)[1:])) + 1] = c
    return torch.from_numpy(out).to(vol_d.device), components


def device_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


class _OnePatient:
    formalized_label_dict = {0: "BG", 1: "LV", 2: "MYO", 3: "RV"}
    patient_number = 1

    def __init__(self, image, label):
        self.pack = {"image": image, "label": label}

    def get_patient_data_for_testing(self, i, crop_size=None):
        return self.pack

    def get_id(self):
        return "p"

    def get_voxel_spacing(self):
        return list(SPACING)


def read_kernel_stats(path):
    calls = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if name.startswith("cc_") or " cc_" in name:
                calls[name.split("(")[0].split()[-1]] = int(row["Calls"])
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cc_postprocess.json"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device-reps", type=int, default=30)
    ap.add_argument("--trace-only", action="store_true", help="one keep_largest_components call per input and nothing else (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --trace-only run under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cc.py measures on the GPU: no device found")
    if args.trace_only:
        for name, vol in inputs():
            ops.keep_largest_components(torch.from_numpy(vol).cuda(), N_CLASS)
        torch.cuda.synchronize()
        print("trace-only: %d calls of keep_largest_components" % len(inputs()))
        return
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import TestSegmentationNetwork, predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=N_CLASS, use_gpu=True)
    solver.eval()
    rows, neighbours = [], {}
    for name, vol in inputs():
        d, h, w = vol.shape
        v = torch.from_numpy(vol).cuda()
        if (d, h, w) not in neighbours:
            gt = torch.from_numpy(phantom(d, h, w, 3, 0)).cuda()
            image = torch.rand(d, 1, h, w, generator=torch.Generator().manual_seed(5))
            image_d = image.cuda()
            _, t_pred, _, _ = timed(lambda: predict_volume(solver, image_d, n_iter=2, chunk=10), args.device_reps, 3)
            ms = runningMySegmentationScore(N_CLASS, metrics_list=["Dice", "HD", "ASD"])
            _, t_upd, _, _ = timed(lambda: ms.update("p", v, gt, voxel_spacing=SPACING), args.device_reps, 3)
            data = _OnePatient(image, gt.cpu())
            scored = {}
            for pp in (None, "largest_cc"):
                t = TestSegmentationNetwork(data, None, solver, metrics_list=("Dice", "HD", "ASD"), keep_results=False, post_process=pp)
                _, scored[pp], _, _ = timed(lambda: t.evaluate(0, data.pack, 1), args.device_reps, 3)
            neighbours[(d, h, w)] = {"predict_volume_ms": t_pred * 1e3, "update_dice_hd_asd_ms": t_upd * 1e3,
                                     "scored_patient_ms": scored[None] * 1e3, "scored_patient_largest_cc_ms": scored["largest_cc"] * 1e3}
        before = _ffi.lib.ctl_launch_count()
        got = ops.keep_largest_components(v, N_CLASS)
        launches = int(_ffi.lib.ctl_launch_count() - before)
        (want, components), t_host, h_lo, h_hi = timed(lambda: host_keep_largest(v), args.host_reps, 1)
        assert torch.equal(got, want), name
        t_dev, d_lo, d_hi = device_ms(lambda: ops.keep_largest_components(v, N_CLASS), args.device_reps)
        _, t_wall, _, _ = timed(lambda: ops.keep_largest_components(v, N_CLASS), args.device_reps, 3)
        assert t_wall < t_host, (name, t_wall, t_host)             # the device path is the faster one on every input
        rec = {"input": name, "volume": [d, h, w], "n_classes": N_CLASS, "form": "3-D, connectivity 1", "components_per_class": components,
               "device_ms": t_dev, "device_ms_min_max": [d_lo, d_hi], "device_wall_ms": t_wall * 1e3, "device_reps": args.device_reps,
               "host_ms": t_host * 1e3, "host_ms_min_max": [h_lo * 1e3, h_hi * 1e3], "host_reps": args.host_reps,
               "host_over_device": t_host * 1e3 / t_dev, "kernel_launches_per_call": launches,
               "post_process_over_predict_volume": t_dev / (neighbours[(d, h, w)]["predict_volume_ms"])}
        rec.update(neighbours[(d, h, w)])
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    by_size = {tuple(r["volume"]): r["device_ms"] for r in rows if r["input"].startswith("phantom")}
    serp = next(r for r in rows if r["input"] == "serpentine")
    ratio = serp["device_ms"] / by_size[tuple(serp["volume"])]
    out = {"what": "ops.keep_largest_components (3-D form, connectivity 1) per volume: device time between HIP events (median, warm) vs the host "
                   "round trip it replaces (copy out, scipy.ndimage.label per class, copy back; wall time); predict_volume = FTN + STN n_iter=2 "
                   "and update = ('Dice', 'HD', 'ASD') on a volume of the same size; scored_patient = TestSegmentationNetwork.evaluate, "
                   "keep_results=False, without and with post_process='largest_cc'",
           "launches": "5 per keep_largest_components call (tiles, merge, flatten, select, output), whatever the volume holds",
           "device_faster_than_host_on_every_input": all(r["device_wall_ms"] < r["host_ms"] for r in rows),
           "serpentine_over_phantom_same_size": ratio, "serpentine_more_than_10x_phantom": ratio > 10.0,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "host_cpus_usable": len(os.sched_getaffinity(0)), "rows": rows}
    if args.kernel_stats:
        out["rocprofv3_kernel_calls"] = {"calls_of_keep_largest_components": len(inputs()), "per_kernel": read_kernel_stats(args.kernel_stats)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
