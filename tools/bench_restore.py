"""Native-grid restoration: the device path (ops.restore_scores) against the host statement it replaces, next to the prediction of the
same volume.

Per volume (raw float32 array, spacing 1.5625 mm resampled to 1.36719 mm in plane, centre crop to 192 x 192, four classes; the scores
are the logits `predict` returns for the prepared volume):
  device    ops.restore_scores on the device-resident logits into a preallocated label volume, HIP events around one call, warm, median
            of repeated calls ("eager"), and the same call captured once into a graph and replayed ("graph"), for both modes, with and
            without the soft output; ops.restore_labels of the window arg-max the same way
  host      prepare.restore_scores_host (numpy) on the same machine, wall time, including the copy of the logits to the host
  predict   tester.predict_volume on the same prepared volume
Nothing is asserted about the times; the labels of both paths are compared where the host's top-two margin exceeds 1e-9 * max |v|.
Writes profiles/restore_volume.json.

    python tools/bench_restore.py [--out profiles/restore_volume.json] [--host-reps 3] [--device-reps 30]
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
from cooperative_training_and_latent_space_data_augmentation_amd import ops, prepare  # noqa: E402

SPACING, NEW_SPACING, CROP = (1.5625, 1.5625, 10.0), [1.36719, 1.36719, -1], [192, 192]
SHAPES = [(10, 256, 216), (40, 256, 256)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_volume.json"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device-reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    rng = np.random.default_rng(0)
    rows = []
    for shape in SHAPES:
        image = rng.random(shape, dtype=np.float32) * 1000
        label = rng.integers(0, 4, size=shape).astype(np.uint8)
        pack = prepare.prepare_patient(image, label, spacing=SPACING, new_spacing=NEW_SPACING, normalize=True, crop_size=CROP,
                                       want_geometry=True)
        geo = pack["geometry"]
        logits = solver.predict(input=pack["image"], softmax=False)
        out = torch.empty(shape, dtype=torch.uint8, device="cuda")
        _, t_pred, p_lo, p_hi = timed(lambda: predict_volume(solver, pack["image"], n_iter=2, chunk=10), args.device_reps, 3)
        rec = {"volume": list(shape), "window": list(geo.window_hw), "resampled": list(geo.resampled_hw), "classes": int(logits.shape[1]),
               "q": list(geo.q), "device_reps": args.device_reps, "host_reps": args.host_reps, "predict_volume_ms": t_pred * 1e3,
               "predict_volume_ms_min_max": [p_lo * 1e3, p_hi * 1e3]}
        for mode in ("logit", "prob"):
            want, t_host, h_lo, h_hi = timed(lambda: prepare.restore_scores_host(logits.float().cpu().numpy(), geo, mode=mode),
                                             args.host_reps, 1)
            v, inside = prepare.restore_values_host(logits.float().cpu().numpy(), geo, mode=mode)
            top2 = np.sort(v, axis=1)[:, -2:]
            decided = ((top2[:, 1] - top2[:, 0]) > 1e-9 * np.abs(v).max()) | ~inside[None]
            got = ops.restore_scores(logits, geo, mode=mode, out=out).cpu().numpy()
            rec[mode] = {"host_statement_ms": t_host * 1e3, "host_statement_ms_min_max": [h_lo * 1e3, h_hi * 1e3],
                         "voxels_under_the_near_tie_bound": int((~decided).sum()),
                         "labels_equal_host_where_decided": bool(np.array_equal(got[decided], want[decided]))}
            for soft in (False, True):
                call = (lambda: ops.restore_scores(logits, geo, mode=mode, want_soft=True, out=out)) if soft else \
                       (lambda: ops.restore_scores(logits, geo, mode=mode, out=out))
                t_dev, d_lo, d_hi = device_ms(call, args.device_reps)
                graph = captured(call)
                t_graph, g_lo, g_hi = device_ms(graph.replay, args.device_reps)
                del graph
                key = "with_soft" if soft else "label_only"
                rec[mode][key] = {"device_eager_ms": t_dev, "device_eager_ms_min_max": [d_lo, d_hi], "device_graph_replay_ms": t_graph,
                                  "device_graph_replay_ms_min_max": [g_lo, g_hi], "over_predict_volume": t_graph / (t_pred * 1e3)}
            rec[mode]["host_over_device_graph_replay_label_only"] = t_host * 1e3 / rec[mode]["label_only"]["device_graph_replay_ms"]
        window_label = ops.argmax_c(logits)
        t_lab, l_lo, l_hi = device_ms(lambda: ops.restore_labels(window_label, geo, out=out), args.device_reps)
        graph = captured(lambda: ops.restore_labels(window_label, geo, out=out))
        t_lab_g, lg_lo, lg_hi = device_ms(graph.replay, args.device_reps)
        del graph
        rec["labels"] = {"device_eager_ms": t_lab, "device_eager_ms_min_max": [l_lo, l_hi], "device_graph_replay_ms": t_lab_g,
                         "device_graph_replay_ms_min_max": [lg_lo, lg_hi],
                         "equal_host": bool(np.array_equal(out.cpu().numpy(), prepare.restore_labels_host(window_label.cpu().numpy(), geo)))}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    res = {"what": "ops.restore_scores (window-grid logits [n,4,192,192] -> native-grid uint8 labels, optionally the float32 soft prediction; "
                   "bilinear in fp64 over the logits or over the per-pixel softmax) per volume on device-resident logits: device time between "
                   "HIP events (median, warm), eager and as the replay of one captured graph; host_statement = prepare.restore_scores_host "
                   "(numpy) wall time on the same machine including the copy of the logits to the host; labels = ops.restore_labels of the "
                   "window arg-max; predict_volume = FTN + STN n_iter=2 on the same prepared volume, wall time",
           "thresholds": "none: nothing was known about these times before this file was written",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "numpy": np.__version__, "host_cpus_usable": len(os.sched_getaffinity(0)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
