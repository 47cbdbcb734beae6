"""Patient volume preparation: the device path (prepare.prepare_patient) against the host statements it replaces, next to the prediction
of the same volume.

Per volume (raw float32 array + uint8 label, spacing 1.5625 mm resampled to 1.36719 mm in plane, 2 / 98 percentile normalisation over
the volume, centre crop to 224 x 224, per-slice rescale):
  device    prepare.prepare_patient on device-resident inputs, HIP events around one call, warm, median of repeated calls ("eager"), and
            the same call captured once into a graph and replayed ("graph")
  normalize ops.percentile_normalize alone on the raw volume (radix select + apply): where the content matters -- a constant volume and a
            volume of 70 % zeros send whole waves to one histogram bin
  host      prepare.prepare_patient_host (numpy) on the same machine, wall time; and the two np.percentile calls of upstream's
            normalize_minmax_data alone
  launches  kernels enqueued per prepare_patient call (the library's census)
and next to them tester.predict_volume on the prepared volume.  Nothing is asserted about the times; the outputs of both paths are
compared.  Writes profiles/prep_volume.json.

    python tools/bench_prep.py [--out profiles/prep_volume.json] [--host-reps 3] [--device-reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface import timed  # noqa: E402
from bench_cc import device_ms  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops, prepare  # noqa: E402

SPACING, NEW_SPACING, CROP = (1.5625, 1.5625, 10.0), [1.36719, 1.36719, -1], [224, 224]


def inputs():
    rng = np.random.default_rng(0)

    def mri(shape):
        x = rng.gamma(2.0, 120.0, size=shape).astype(np.float32)
        x[rng.random(shape) < 0.7] = 0
        return x
    return [("random", rng.random((10, 256, 216), dtype=np.float32) * 1000), ("MRI-like, 70 % zeros + gamma tail", mri((10, 256, 216))),
            ("constant", np.zeros((10, 256, 216), dtype=np.float32)), ("random", rng.random((40, 256, 256), dtype=np.float32) * 1000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_volume.json"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device-reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prep.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    kw = dict(spacing=SPACING, new_spacing=NEW_SPACING, normalize=True, crop_size=CROP)
    rows = []
    for name, image in inputs():
        label = (np.random.default_rng(1).integers(0, 4, size=image.shape)).astype(np.uint8)
        image_d, label_d = torch.from_numpy(image).cuda(), torch.from_numpy(label).cuda()
        before = _ffi.lib.ctl_launch_count()
        got = prepare.prepare_patient(image_d, label_d, **kw)
        launches = int(_ffi.lib.ctl_launch_count() - before)
        want, t_host, h_lo, h_hi = timed(lambda: prepare.prepare_patient_host(image, label, **kw), args.host_reps, 1)
        same_label = bool(np.array_equal(got["label"].cpu().numpy(), want["label"]))
        g = got["image"].cpu().numpy()
        both_nan = np.isnan(g) & np.isnan(want["image"])
        same_image = bool(((g.view(np.uint32) == want["image"].view(np.uint32)) | both_nan).all())
        _, t_pct, _, _ = timed(lambda: (np.percentile(image, 2), np.percentile(image, 98)), args.host_reps, 1)
        t_dev, d_lo, d_hi = device_ms(lambda: prepare.prepare_patient(image_d, label_d, **kw), args.device_reps)
        _, t_wall, _, _ = timed(lambda: prepare.prepare_patient(image_d, label_d, **kw), args.device_reps, 3)
        t_norm, n_lo, n_hi = device_ms(lambda: ops.percentile_normalize(image_d, (2.0, 98.0)), args.device_reps)
        t_sel, _, _ = device_ms(lambda: ops.order_statistics(image_d, [11058, 11059, 541900, 541901]), args.device_reps)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            prepare.prepare_patient(image_d, label_d, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pack = prepare.prepare_patient(image_d, label_d, **kw)
        t_graph, g_lo, g_hi = device_ms(graph.replay, args.device_reps)
        assert torch.equal(pack["label"], got["label"])
        _, t_pred, _, _ = timed(lambda: predict_volume(solver, got["image"], n_iter=2, chunk=10), args.device_reps, 3)
        rec = {"input": name, "volume": list(image.shape), "prepared": list(got["image"].shape), "device_eager_ms": t_dev,
               "device_eager_ms_min_max": [d_lo, d_hi], "device_eager_wall_ms": t_wall * 1e3, "device_graph_replay_ms": t_graph,
               "device_graph_replay_ms_min_max": [g_lo, g_hi], "percentile_normalize_ms": t_norm, "percentile_normalize_ms_min_max": [n_lo, n_hi],
               "order_statistics_4_ranks_ms": t_sel, "device_reps": args.device_reps, "host_statement_ms": t_host * 1e3,
               "host_statement_ms_min_max": [h_lo * 1e3, h_hi * 1e3], "host_np_percentile_2_98_ms": t_pct * 1e3, "host_reps": args.host_reps,
               "host_over_device_eager": t_host * 1e3 / t_dev, "kernel_launches_per_call": launches, "predict_volume_ms": t_pred * 1e3,
               "prepare_over_predict_volume": t_dev / (t_pred * 1e3), "labels_equal_host": same_label, "image_bits_equal_host": same_image}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del graph, pack
    out = {"what": "prepare.prepare_patient (resample in plane, 2 / 98 percentile normalisation over the volume, centre crop, per-slice rescale) "
                   "per volume on device-resident inputs: device time between HIP events (median, warm), eager and as the replay of one "
                   "captured graph; percentile_normalize = radix select + apply alone on the raw volume; host_statement = "
                   "prepare.prepare_patient_host (numpy) wall time on the same machine; host_np_percentile_2_98 = the two np.percentile "
                   "calls of normalize_minmax_data on the float32 volume; predict_volume = FTN + STN n_iter=2 on the prepared volume",
           "thresholds": "none: nothing was known about these times before this file was written",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "numpy": np.__version__, "host_cpus_usable": len(os.sched_getaffinity(0)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
