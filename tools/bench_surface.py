"""Patient scoring with surface metrics: host (scipy) path against the device path, next to the prediction it scores.

For the two phantom sizes of tests/test_surface_gpu.py (10x192x192 and 40x256x256, 4 classes) and the metric lists
("Dice", "HD"), ("Dice", "HD", "ASD") and ("Dice", "HD", "HD95", "ASD", "ASSD") this times, per patient,
  host    what `runningMySegmentationScore.update` did for device volumes before the device path existed: voxel counts from the
          confusion-matrix kernel, both label volumes copied to the host, scipy erosion + distance transform per class / direction / slice
  device  `update` as it is now (ops.surface_stats, one readback of the small tables)
  predict `tester.predict_volume` on a volume of the same size (FTN + STN, n_iter = 2, eval BatchNorm, arg-max)
each as the median over repeated calls after a warm-up, with a device synchronise on both sides of every timed call, checks that
both paths return the same row, and writes profiles/surface_metrics.json.

With --quantile-reps N > 0 (the default) it also times, on the same volumes, `ops.surface_quantiles` alone (per-slice form, q = 95, with
the statistics table: what 'HD' + 'HD95' cost together) beside `ops.surface_stats` alone (what 'HD' costs), each as an eager call and as
the replay of a captured graph with caller-owned buffers, and records their ratio: the fused call has to stay below two statistics
calls.  The device times of the file it overwrites (the parent's numbers) are carried along as `parent_device_ms`.

    python tools/bench_surface.py [--out profiles/surface_metrics.json] [--host-reps 3] [--device-reps 30] [--quantile-reps 30]
"""
import argparse
import ctypes
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

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, metrics, ops  # noqa: E402
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
            elif m == "HD95":
                row.append(float(metrics.hd95_2D_stack(p_h == c, g_h == c, pixelspacing=spacing[:2], connectivity=2)))
            elif m == "ASSD":
                row.append(float(metrics.assd(p_h == c, g_h == c, voxelspacing=spacing, connectivity=2)))
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


def timed_alternating(fns, reps, warmup):
    """`timed` for several callables measured in turn inside one loop, so that drift of the machine hits them alike."""
    outs = [None] * len(fns)
    for _ in range(warmup):
        outs = [fn() for fn in fns]
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[k] = fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return [(o, statistics.median(t), min(t), max(t)) for o, t in zip(outs, times)]


def graph_of(call):
    """Capture `call` (launches on the current stream into buffers allocated beforehand) once; -> the replay function."""
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    return graph.replay


def quantile_record(pr, gt, reps):
    """ops.surface_quantiles (2-D form, q = 95, with the statistics table) against ops.surface_stats on one patient."""
    d, h, w = (int(v) for v in pr.shape)
    sp = SPACING[:2]
    ((qt, st), t_q, q_lo, q_hi), (ref, t_s, s_lo, s_hi) = timed_alternating(
        [lambda: ops.surface_quantiles(pr, gt, N_CLASS, (95.0,), sp, 2, "2d", want_stats=True), lambda: ops.surface_stats(pr, gt, N_CLASS, sp, 2, "2d")],
        reps, 3)
    assert torch.equal(st, ref)
    # the same two calls with caller-owned buffers, captured once and replayed
    p8, g64 = pr.to(torch.uint8).contiguous(), gt.long().contiguous()
    samp, qa = (ctypes.c_double * 2)(*sp), (ctypes.c_double * 1)(95.0)
    nb_q = _ffi.lib.ctl_surface_quantiles_ws_bytes(d, h, w, N_CLASS, 0, 2, 1)
    nb_s = _ffi.lib.ctl_surface_stats_ws_bytes(d, h, w, N_CLASS, 0, 2)
    ws_q, ws_s = (torch.empty(n, dtype=torch.uint8, device=pr.device) for n in (nb_q, nb_s))
    qt_g, st_g, ref_g = torch.empty_like(qt), torch.empty_like(st), torch.empty_like(ref)

    def call_q():
        _ffi.check(_ffi.lib.ctl_surface_quantiles(p8.data_ptr(), g64.data_ptr(), d, h, w, N_CLASS, 0, 2, 2, samp, qa, 1, st_g.data_ptr(),
                                                  qt_g.data_ptr(), ws_q.data_ptr(), nb_q, ops.stream_ptr()), "ctl_surface_quantiles")

    def call_s():
        _ffi.check(_ffi.lib.ctl_surface_stats(p8.data_ptr(), g64.data_ptr(), d, h, w, N_CLASS, 0, 2, 2, samp, ref_g.data_ptr(), ws_s.data_ptr(),
                                              nb_s, ops.stream_ptr()), "ctl_surface_stats")

    (_, t_qg, qg_lo, qg_hi), (_, t_sg, sg_lo, sg_hi) = timed_alternating([graph_of(call_q), graph_of(call_s)], reps, 3)
    assert torch.equal(qt_g.view(torch.int64), qt.view(torch.int64)) and torch.equal(st_g, ref) and torch.equal(ref_g, ref)
    return {"volume": [d, h, w], "n_classes": N_CLASS, "mode": "2d", "q": [95.0], "want_stats": True, "reps": reps,
            "surface_quantiles_ms": t_q * 1e3, "surface_quantiles_ms_min_max": [q_lo * 1e3, q_hi * 1e3],
            "surface_stats_ms": t_s * 1e3, "surface_stats_ms_min_max": [s_lo * 1e3, s_hi * 1e3],
            "quantiles_over_stats": t_q / t_s,
            "surface_quantiles_graph_ms": t_qg * 1e3, "surface_quantiles_graph_ms_min_max": [qg_lo * 1e3, qg_hi * 1e3],
            "surface_stats_graph_ms": t_sg * 1e3, "surface_stats_graph_ms_min_max": [sg_lo * 1e3, sg_hi * 1e3],
            "quantiles_over_stats_graph": t_qg / t_sg, "pooled_keys": int(qt[..., 2].sum().item()), "groups": int(qt.shape[0] * qt.shape[1])}


def parent_device_ms(path):
    """{(volume, metrics): device_ms} of the file about to be overwritten."""
    try:
        with open(path) as f:
            return {(tuple(r["volume"]), tuple(r["metrics"])): r["device_ms"] for r in json.load(f)["rows"]}
    except (OSError, ValueError, KeyError):
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics.json"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device-reps", type=int, default=30)
    ap.add_argument("--quantile-reps", type=int, default=30, help="repetitions of the ops.surface_quantiles / ops.surface_stats section; 0 skips it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=N_CLASS, use_gpu=True)
    solver.eval()
    rows, quantiles, parent = [], [], parent_device_ms(args.out)
    for d, h, w in ((10, 192, 192), (40, 256, 256)):
        pr = torch.from_numpy(phantom(d, h, w, 6, 1).astype(np.uint8)).cuda()
        gt = torch.from_numpy(phantom(d, h, w, 3, 0)).cuda()
        image = torch.rand(d, 1, h, w, generator=torch.Generator().manual_seed(5)).cuda()
        _, t_pred, _, _ = timed(lambda: predict_volume(solver, image, n_iter=2, chunk=10), args.device_reps, 3)
        if args.quantile_reps > 0:
            quantiles.append(quantile_record(pr, gt, args.quantile_reps))
            quantiles[-1]["predict_volume_ms"] = t_pred * 1e3
            print(json.dumps(quantiles[-1]), flush=True)
        for mlist in (("Dice", "HD"), ("Dice", "HD", "ASD"), ("Dice", "HD", "HD95", "ASD", "ASSD")):
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
            if ((d, h, w), tuple(mlist)) in parent:
                rec["parent_device_ms"] = parent[((d, h, w), tuple(mlist))]
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    out = {"what": "runningMySegmentationScore.update per patient: surface metrics on the host (scipy, after copying both label volumes) vs on "
                   "the device (ops.surface_stats); medians of wall time around device synchronises; predict_volume = FTN + STN n_iter=2 on "
                   "a volume of the same size",
           "launches": "2 (confusion matrices) + 4 per 'HD' (per-slice 2-D form; 7 for 'HD' with 'HD95': ops.surface_quantiles) + 5 per 'ASD' "
                       "and / or 'ASSD' (3-D form), independent of slices and classes",
           "quantiles": quantiles,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip, "torch": torch.__version__, "host": platform.node(),
           "host_cpus_usable": len(os.sched_getaffinity(0)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
