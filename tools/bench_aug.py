"""Training augmentation of one batch: the device path (augment.BatchAugmenter.apply) against the host path it replaces and against the
training step it feeds.

Batches of 16 slices, policy ACDC_affine_elastic_intensity, 224x224 -> 192x192 and 256x256 -> 256x256.  Per size two rows: the parameters
as the policy draws them (elastic on for about half of the samples) and elastic forced on for all 16 (the worst case); each row once per
interpolation of --interp (linear: bilinear image / nearest label; cubic: cubic spline for both, 4 classes; both: the two side by side
from the same run, on the same batch and parameters).  Per row:
  device   HIP events around one apply() on an idle stream, warm, median of repeated calls; eagerly and as the replay of a captured graph
  host     augment.apply_host on the same batch and parameters (fp64 numpy / scipy, one sample after the other: scipy.ndimage does not
           thread); wall time, with the number of CPUs the process may use
  launches kernels enqueued per apply() (the library's census)
  share    device time / step time, for every step time given with --step-line (the JSON line of a `bench.py` run of the same session)
Checks that device and host agree on the labels of the first row, and writes profiles/aug_batch.json.
--config v2 / coarse measures a config-dict chain (BatchAugmenter.from_config) in place of the policy: upstream's ACDC_affine_all config
(bias field + Gaussian elastic + intensity) or its ACDC_affine_elastic_intensity_v2 config (coarse-grid elastic + intensity); the
"forced" row then sets the probabilities of those stages to 1.

    python bench.py --gpus 1 --steps 20 --warmup 5 > step_fp32.json
    python tools/bench_aug.py --interp both --step-line step_fp32.json [--step-line step_bf16.json] [--out profiles/aug_batch.json]
    python tools/bench_aug.py --config v2 --interp linear --out profiles/aug_batch_v2.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, augment  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter  # noqa: E402

POLICY = "ACDC_affine_elastic_intensity"
N = 16
SIZES = [((224, 224), (192, 192)), ((256, 256), (256, 256))]
CLASSES = 4                      # batch() draws the labels 0..3
CONFIGS = {"v2": "ACDC_affine_all", "coarse": "ACDC_affine_elastic_intensity_v2"}       # --config: the upstream config each choice measures


def make_augmenter(choice, forced, crop, interp):
    """(augmenter, what it is called) for one row."""
    kw = dict(seed=0, interp=interp, num_classes=CLASSES if interp == "cubic" else None)
    if choice == "policy":
        return BatchAugmenter(POLICY, crop, **kw), POLICY
    config = augment.reference_config(CONFIGS[choice])
    if forced:
        for k in ("elastic_prob", "elastic_probv2", "perturb_v2_prob"):
            config[k] = 1.0 if config[k] > 0 else config[k]
    return BatchAugmenter.from_config(config, crop, **kw), "config of " + CONFIGS[choice]


def batch(n, hp, wp, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:hp, 0:wp]
    image = np.zeros((n, 1, hp, wp), dtype=np.float32)
    label = np.zeros((n, hp, wp), dtype=np.int64)
    for b in range(n):
        for c in (1, 2, 3):
            cy, cx, r = rng.uniform(0.3, 0.7) * hp, rng.uniform(0.3, 0.7) * wp, rng.uniform(0.08, 0.2) * hp
            d2 = (y - cy) ** 2 + (x - cx) ** 2
            image[b, 0] += np.exp(-d2 / (2 * r * r)).astype(np.float32)
            label[b][d2 < r * r] = c
    return image + 0.05 * rng.standard_normal(image.shape).astype(np.float32), label


def device_ms(fn, reps, warmup=5):
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


def read_step_lines(paths):
    steps = []
    for path in paths:
        with open(path) as f:
            for line in f:
                line = line.strip()
                if line.startswith("{") and "ms_per_step" in line:
                    rec = json.loads(line)
                    steps.append({"file": os.path.basename(path), "dtype": rec.get("dtype"), "mode": rec.get("mode"),
                                  "ms_per_step": rec["ms_per_step"], "slices_per_s": rec.get("value"),
                                  "batch": (rec.get("config") or {}).get("global_batch")})
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_batch.json"))
    ap.add_argument("--device-reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--interp", choices=("linear", "cubic", "both"), default="both")
    ap.add_argument("--config", choices=("policy",) + tuple(CONFIGS), default="policy",
                    help="policy: BatchAugmenter(%s); v2 / coarse: from_config of upstream's %s / %s config" % ((POLICY,) + tuple(CONFIGS.values())))
    ap.add_argument("--step-line", action="append", default=[], help="file holding the JSON line of a bench.py run of this session")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_aug.py measures on the GPU: no device found")
    steps = read_step_lines(args.step_line)
    interps = ("linear", "cubic") if args.interp == "both" else (args.interp,)
    rows = []
    for (hp, wp), crop in SIZES:
        image_h, label_h = batch(N, hp, wp, 1)
        image, label = torch.from_numpy(image_h).cuda(), torch.from_numpy(label_h).cuda()
        for forced, interp in ((f, i) for f in (False, True) for i in interps):
            aug, what = make_augmenter(args.config, forced, crop, interp)
            p = aug.draw(N, hp, wp)
            if forced and args.config == "policy":
                off = p["alpha"] == 0
                p["alpha"][off] = float(np.float32(1.75 * hp))
                p["elastic_on"][:] = True
            pd = aug.upload(p, image.device)
            before = _ffi.lib.ctl_launch_count()
            got_i, got_l = aug.apply(image, label, pd)
            launches = int(_ffi.lib.ctl_launch_count() - before)
            eager = device_ms(lambda: aug.apply(image, label, pd), args.device_reps)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                g_i, g_l = aug.apply(image, label, pd)
            replay = device_ms(graph.replay, args.device_reps)
            assert torch.equal(g_i, got_i) and torch.equal(g_l, got_l)
            t_wall0 = time.perf_counter()
            for _ in range(args.device_reps):
                aug.apply(image, label, pd)
            torch.cuda.synchronize()
            wall_ms = (time.perf_counter() - t_wall0) * 1e3 / args.device_reps
            host = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                want_i, want_l = augment.apply_host(image_h, label_h, p, interp=interp, n_class=aug.num_classes)
                host.append((time.perf_counter() - t0) * 1e3)
            host_ms = statistics.median(host)
            agree = float((got_l.cpu().numpy() == want_l).mean())
            assert agree > 0.97, agree         # the fp32 / fp64 displacements differ by up to 4e-5 * alpha px: labels on a rounding boundary
            on = {k: (None if p.get(k) is None else int(p[k].sum())) for k in ("bias_on", "coarse_on")}
            rec = {"policy": what, "interp": interp, "n_class": aug.num_classes, "batch": N, "input": [hp, wp], "crop": list(crop), "elastic_samples": int(p["elastic_on"].sum()),
                   "bias_samples": on["bias_on"], "coarse_samples": on["coarse_on"],
                   "elastic_forced_on": forced, "sigma_px_max": None if p["sigma"] is None else float(p["sigma"].max()), "device_eager_ms": eager[0],
                   "device_eager_ms_min_max": [eager[1], eager[2]], "device_graph_replay_ms": replay[0],
                   "device_graph_replay_ms_min_max": [replay[1], replay[2]], "device_eager_wall_ms": wall_ms, "device_reps": args.device_reps,
                   "kernel_launches_per_batch": launches, "host_ms": host_ms, "host_ms_per_slice": host_ms / N, "host_reps": args.host_reps,
                   "host_threads": 1, "host_over_device_graph": host_ms / replay[0], "host_over_device_eager": host_ms / eager[0],
                   "label_agreement_with_host": agree,
                   "share_of_step": [{**s, "graph_replay_share": replay[0] / s["ms_per_step"], "eager_share": eager[0] / s["ms_per_step"],
                                      "host_over_step": host_ms / s["ms_per_step"]} for s in steps]}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    out = {"what": "augment.BatchAugmenter.apply on one batch of 16 slices (ctl_aug_field 2 launches, ctl_aug_warp 2 or ctl_aug_warp_cubic 4, "
                   "ctl_rescale_intensity 2; with --config v2 ctl_aug_bias 2 more, with --config coarse ctl_aug_coarse_field 1 in place of ctl_aug_field): "
                   "device time between HIP events (median, warm), eager and as a graph replay, vs augment.apply_host (fp64 numpy / scipy) on "
                   "the same batch and parameters, and as a share of the training step of the bench.py runs of the same session",
           "launches": "6 per batch with an elastic policy (8 with interp cubic), whatever n is", "interp": list(interps), "config": args.config, "steps": steps,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "host_cpus_usable": len(os.sched_getaffinity(0)), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
