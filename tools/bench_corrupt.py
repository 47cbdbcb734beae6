"""MR artefact corruption of a test volume (corrupt.corrupt_volume: RandomBias, RandomSpike, RandomGhosting, RandomMotion) on the
device, against the fp64 host statements it is defined by, next to the prediction of the same volume.

Per kind and volume (10 x 192 x 192 and 40 x 256 x 256, non-negative in [0, 1], parameters drawn from seed 0; for RandomGhosting once per
axis, since the operator runs along another stride on each):
  device    a corrupt.Corruption made once (operator matrix, workspace and the stack of rigid copies live on the device), HIP events
            around one call, warm, median of repeated calls ("eager"), and the same call captured once into a graph and replayed
            ("graph"); and corrupt.corrupt_volume as a user calls it (parameters -> operator on the host -> upload -> kernels -> per-slice
            rescale), wall time
  host      the `*_host` statement (numpy, fp64) on the same machine, wall time
  launches  kernels enqueued per call (the library's census)
and next to them tester.predict_volume on the same volume.  Nothing is asserted about the times; the largest difference between the
device result and the host statement is recorded.  Writes profiles/corrupt_volume.json.

    python tools/bench_corrupt.py [--out profiles/corrupt_volume.json] [--host-reps 2] [--device-reps 30]
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
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, corrupt  # noqa: E402

SHAPES = [(10, 192, 192), (40, 256, 256)]


def volume(shape):
    rng = np.random.default_rng(0)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    blob = np.exp(-2.0 * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2))
    return np.clip(0.7 * blob + 0.3 * rng.uniform(0, 1, shape), 0, 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corrupt_volume.json"))
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--device-reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corrupt.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    rows = []
    for shape in SHAPES:
        x = volume(shape)
        x_d = torch.from_numpy(x).cuda()
        _, t_pred, _, _ = timed(lambda: predict_volume(solver, x_d[:, None], n_iter=2, chunk=10), args.device_reps, 3)
        cases = []
        for kind in corrupt.KINDS:
            p = corrupt.draw_parameters(kind, shape, np.random.default_rng(0))
            if kind == "RandomGhosting":
                cases += [(kind, dict(p, axis=a)) for a in (0, 1, 2)]
            else:
                cases.append((kind, p))
        for kind, p in cases:
            f = corrupt.Corruption(kind, p, shape)
            before = _ffi.lib.ctl_launch_count()
            got = f(x_d)
            launches = int(_ffi.lib.ctl_launch_count() - before)
            want, t_host, h_lo, h_hi = timed(lambda: corrupt.corrupt_volume_host(x, kind, p, rescale=False), args.host_reps, 0)
            diff = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
            t_dev, d_lo, d_hi = device_ms(lambda: f(x_d), args.device_reps)
            _, t_wall, _, _ = timed(lambda: corrupt.corrupt_volume(x_d, kind, p), args.device_reps, 3)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                f(x_d)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            out = torch.empty(shape, device="cuda")
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                f(x_d, out=out)
            t_graph, g_lo, g_hi = device_ms(graph.replay, args.device_reps)
            same = bool(torch.equal(out, got))
            rec = {"kind": kind, "volume": list(shape), "axis": p.get("axis"), "device_eager_ms": t_dev, "device_eager_ms_min_max": [d_lo, d_hi],
                   "device_graph_replay_ms": t_graph, "device_graph_replay_ms_min_max": [g_lo, g_hi], "corrupt_volume_wall_ms": t_wall * 1e3,
                   "device_reps": args.device_reps, "host_statement_ms": t_host * 1e3, "host_statement_ms_min_max": [h_lo * 1e3, h_hi * 1e3],
                   "host_reps": args.host_reps, "host_over_device_eager": t_host * 1e3 / t_dev, "kernel_launches_per_call": launches,
                   "predict_volume_ms": t_pred * 1e3, "corrupt_over_predict_volume": t_dev / (t_pred * 1e3),
                   "max_abs_difference_from_host_statement": diff, "graph_replay_bits_equal_eager": same}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            del graph, out, f
    res = {"what": "one corruption of one device-resident volume with fixed parameters (corrupt.Corruption): device time between HIP events "
                   "(median, warm), eager and as the replay of one captured graph; corrupt_volume_wall = corrupt.corrupt_volume including "
                   "the host's operator matrix, its upload and the per-slice rescale; host_statement = the fp64 numpy statement "
                   "(corrupt.corrupt_volume_host, no rescale) wall time on the same machine; predict_volume = FTN + STN n_iter=2 on the "
                   "same volume",
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
