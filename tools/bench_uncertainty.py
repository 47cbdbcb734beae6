"""Predictive-uncertainty kernel (csrc/ctl_uncert.hip) at volume sizes: logits 10 x 4 x 192 x 192 and 40 x 4 x 256 x 256 per member,
T = 1 and 2 members, a label volume, 15 bins, the entropy map and both tables written (what the tester asks for with
uncertainty_maps=True is one map more).

Per size and T:
  eager / graph   device time of ops.predictive_stats between HIP events, warm, median over repeated batches of `--inner` calls divided
                  by the batch: the calls as issued from Python, and the replay of one captured graph
  aten_eager      the same quantities (entropy map, per-slice sums, reliability bins by bucketize + a one-hot sum) composed from ATen
                  ops on the device
  numpy           the float64 host statement (uncertainty.predictive_stats_host) on this machine's CPU, INCLUDING the copy of the logits
                  to the host: what a user had to do before
  bytes           what the algorithm must move: T * n * hw * C * 4 (logits) + n * hw * 8 (labels) + n * hw * 4 (entropy map);
                  bytes / graph time against the achievable HBM rate of 6.3 TB/s (8 TB/s peak)
  predict_volume  device time of tester.predict_volume on a volume of the same size (T = 1), and the kernel's cost relative to it
The device result is compared with the host statement at the smaller size and the errors recorded.  Nothing is asserted about the times.
Writes profiles/uncertainty.json.

    python tools/bench_uncertainty.py [--out profiles/uncertainty.json] [--reps 20] [--inner 20] [--host-reps 3]
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
from cooperative_training_and_latent_space_data_augmentation_amd import ops, uncertainty  # noqa: E402

SIZES = [(10, 4, 192, 192), (40, 4, 256, 256)]
BINS, EPS = 15, 1e-7
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12


def aten_stats(x, y, t, n_bins=BINS, eps=EPS):
    """entropy map, stats [n,6] and bins [n,B,3] from ATen ops on the device"""
    tn, c, h, w = x.shape
    n = tn // t
    p = torch.softmax(x.view(t, n, c, h, w), 2)
    pbar = p.mean(0)
    ent = -(pbar * torch.log2(pbar + eps)).sum(1)
    mi = ent - (-(p * torch.log2(p + eps)).sum(2)).mean(0) if t > 1 else torch.zeros_like(ent)
    conf, pred = pbar.max(1)
    valid = (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    py = pbar.gather(1, yc.unsqueeze(1)).squeeze(1)
    nll = torch.where(valid, -torch.log(py), torch.zeros_like(py)).double()
    brier = torch.where(valid, ((pbar - torch.nn.functional.one_hot(yc, c).permute(0, 3, 1, 2)) ** 2).sum(1), torch.zeros_like(py)).double()
    correct = valid & (pred == y)
    stats = torch.stack([valid.sum((1, 2)).double(), correct.sum((1, 2)).double(), ent.double().sum((1, 2)), mi.double().sum((1, 2)),
                         nll.sum((1, 2)), brier.sum((1, 2))], 1)
    edges = torch.arange(1, n_bins, device=x.device, dtype=torch.float32) / n_bins
    which = torch.bucketize(conf, edges, right=False)                                                           # edges with conf > edge
    hot = (which.unsqueeze(-1) == torch.arange(n_bins, device=x.device)) & valid.unsqueeze(-1)                  # [n,h,w,B]
    bins = torch.stack([hot.sum((1, 2)).double(), (hot & correct.unsqueeze(-1)).sum((1, 2)).double(),
                        (hot * conf.unsqueeze(-1).double()).sum((1, 2))], -1)
    return ent, stats, bins


def per_call(fn, reps, inner):
    med, lo, hi = device_ms(lambda: [fn() for _ in range(inner)], reps)
    return {"ms": med / inner, "ms_min_max": [lo / inner, hi / inner]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncertainty.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    rows = {}
    for n, c, h, w in SIZES:
        g = torch.Generator().manual_seed(n)
        y = torch.randint(0, c, (n, h, w), generator=g)
        yd = y.cuda()
        image = torch.rand(n, 1, h, w, generator=g).cuda()
        pv = per_call(lambda: predict_volume(solver, image), max(args.reps // 4, 3), 2)
        for t in (1, 2):
            x = (torch.randn(t * n, h, w, c, generator=g) * 3.0).permute(0, 3, 1, 2)
            xd = x.cuda()
            fused = lambda: ops.predictive_stats(xd, yd, members=t, n_bins=BINS, eps=EPS, want=("entropy",))      # noqa: E731
            rec = {"eager": per_call(fused, args.reps, args.inner)}
            graph = captured(fused)
            rec["graph"] = per_call(graph.replay, args.reps, args.inner)
            del graph
            rec["aten_eager"] = per_call(lambda: aten_stats(xd, yd, t), args.reps, max(args.inner // 4, 2))
            host = []
            for _ in range(args.host_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = uncertainty.predictive_stats_host(xd.cpu().numpy(), y.numpy(), members=t, n_bins=BINS, eps=EPS)
                host.append((time.perf_counter() - t0) * 1e3)
            rec["numpy_with_copy"] = {"ms": float(np.median(host)), "ms_min_max": [min(host), max(host)]}
            nbytes = t * n * h * w * c * 4 + n * h * w * 8 + n * h * w * 4
            rate = nbytes / (rec["graph"]["ms"] * 1e-3)
            rec["bytes"] = nbytes
            rec["bytes_per_s_graph"] = rate
            rec["share_of_achievable_hbm"] = rate / HBM_ACHIEVABLE
            rec["share_of_peak_hbm"] = rate / HBM_PEAK
            rec["aten_eager_over_graph"] = rec["aten_eager"]["ms"] / rec["graph"]["ms"]
            rec["numpy_over_graph"] = rec["numpy_with_copy"]["ms"] / rec["graph"]["ms"]
            if t == 1:
                rec["predict_volume"] = pv
                rec["graph_over_predict_volume"] = rec["graph"]["ms"] / pv["ms"]
            if n == SIZES[0][0]:
                got = fused()
                cal_d = uncertainty.calibration_from_tables(got.stats.cpu().numpy(), got.bins.cpu().numpy(), pixels=y.numel())
                cal_h = uncertainty.calibration_from_tables(ref.stats, ref.bins, pixels=y.numel())
                rec["entropy_map_max_abs_error"] = float(np.abs(got.entropy.cpu().numpy() - ref.entropy).max())
                rec["column_abs_errors"] = {k: abs(cal_d[k] - cal_h[k]) for k in uncertainty.CALIBRATION_METRICS}
            rows[f"{n}x{c}x{h}x{w} T={t}"] = rec
            print(json.dumps({f"{n}x{c}x{h}x{w} T={t}": rec}), flush=True)
    res = {"what": "ops.predictive_stats (entropy map + stats + bins, 15 bins, labels given) on fp32 NHWC logits [T*n, C, H, W]: device time "
                   f"between HIP events per call (median of {args.reps} batches of {args.inner} calls, warm), eager and as the replay of one captured "
                   "graph; aten_eager = the same quantities from ATen ops; numpy_with_copy = the float64 host statement including the copy of the "
                   "logits to the host (wall time); bytes = logits + labels + entropy map; predict_volume = tester.predict_volume on a volume "
                   "of the same size (random weights, FCN_16_standard)",
           "thresholds": "none", "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "hbm_peak_bytes_per_s": HBM_PEAK,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
