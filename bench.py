#!/usr/bin/env python3
"""Headline benchmark: cooperative-training slices/s on synthetic 256x256 batches (BASELINE.json configs[1]):
batch 16 per GPU, full cooperative step = standard_training + hard_example_generation (dropout masks on both latent
codes) + hard_example_training + backward + 5x Adam, fp32, one process per GPU.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run does only what the headline figure needs: set-up, W warm-up steps, the execution-mode calibration (`--mode auto`),
K timed steps, the outputs of the last timed step if `--dump-outputs DIR` is given, and the result line.  `--full` adds everything
else this script measures, each in runs of its own behind the timed region (or, for the sampled dominant kernel, inside it):

    python bench.py --gpus 1 --steps 20 --warmup 5 --full

The LAST line of stdout (rank 0) is ONE JSON object of at most 3 KB (`headline()` below): the driver's contract keys (`ms_per_step`:
wall time of one timed step) and `roofline_step` (the whole step against its floor, from `ms_per_step` alone); with `--full` also
`roofline` of the kernel with the largest serial time in the step (arg-max of the per-launch HIP-event profile, measured live on the
launch stream), `cpu_baseline` (the CPU oracle oracle/ref_cpu.py, a port of the reference's PyTorch-CPU path, timed on one step
of the same workload on the host cores, N=1 only) and, at N=1, three sub-records cut down to seven numbers each: `config3_bf16`
(BASELINE configs[2]: targeted masks, bf16), `config5_inference` (configs[4]: 192x192 volume inference) and `config4_random_masks_n1`
(configs[3]'s masking scheme -- all three schemes randomly sampled -- on one GPU), measured by child processes running this same script.  Everything else (per-family / per-kernel rooflines, per-step times, allocation
counters, mode calibration, the full sub-records) goes to `bench_detail.json` next to this script and, as one line prefixed
`BENCH_DETAIL `, to stderr -- stdout carries nothing but the headline line.

`--dump-outputs DIR` writes what the timed path computed in its last timed step as DIR/<name>.npy (float32 / float64): the 8 losses
the step returns, the latent masks it drew, and every network's weights and BatchNorm buffers after its Adam update (inference: the
label volume).  Inputs, initial weights and the host RNG streams are seeded, so runs with the same arguments start from identical
inputs; the dropout draws of an eager step and of a graph replay differ, so pin `--mode` when two builds' outputs are compared."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DROP_IMG = {"loss_name": "mse", "mask_type": "dropout", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
DROP_SEG = {"loss_name": "ce", "mask_type": "dropout", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
TGT_IMG = {"loss_name": "mse", "mask_type": "channel", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
TGT_SEG = {"loss_name": "ce", "mask_type": "spatial", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
RND_IMG = {"loss_name": "mse", "mask_type": "random", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
RND_SEG = {"loss_name": "ce", "mask_type": "random", "max_threshold": 0.5, "random_threshold": True, "if_soft": True}
MASKS = {"dropout": (DROP_IMG, DROP_SEG, "dropout latent masks"),                      # BASELINE configs[1]
         "targeted": (TGT_IMG, TGT_SEG, "targeted channel-wise (image code) + spatial-wise (shape code) masks: extra dL/dz backward + top-k"),   # configs[2]
         "random": (RND_IMG, RND_SEG, "all three masking schemes randomly sampled per step")}                                                  # configs[3]
PEAK_MFMA_F32_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak
PEAK_MFMA_BF16_TFLOPS = 2500.0   # MI355X_MICROARCH.md: dense bf16 MFMA peak
PEAK_HBM_GBS = 8000.0
# whole-step floors (SURVEY 8(d) / BASELINE.md section 4, ideal fusion: every conv reads its input once and writes its output once, fp32):
# GB per slice of the full step by masking scheme; bf16 storage halves it.  flops: conv MACs x 2 per slice.
STEP_GB_PER_SLICE = {"dropout": 2.110, "targeted": 2.209, "random": 2.176}      # random: dropout / channel / spatial with probability 1/3 each per code
STEP_GFLOP_PER_SLICE = {"dropout": 77.9, "targeted": 83.6, "random": 81.7}
X3_PRODUCTS = 6                  # an X3 launch (fp32 operands split exactly into three bf16 numbers, csrc/ctl_conv_x3_stage.h) issues six bf16 MFMA
                                 # products per fp32 product: its matrix-side ceiling for ALGORITHMIC flops is the bf16 peak / 6 = 416.7 TFLOP/s


def peak_mfma_of(kernel_id, dtype):
    """dense matrix peak, in algorithmic TFLOP/s, of the pipe a profiling id runs on"""
    if dtype == "bf16":
        return PEAK_MFMA_BF16_TFLOPS
    if kernel_id.startswith(("conv_igemm_x3", "conv_wgrad_x3")):
        return PEAK_MFMA_BF16_TFLOPS / X3_PRODUCTS
    return PEAK_MFMA_F32_TFLOPS
# the dominant kernel is not a constant: it is the profiling id with the largest serial time in a single-stream replay of the step
# (every launch bracketed with HIP events on its launch stream), picked before the timed region and re-measured behind it
PROF_EVERY = 4                   # inside the timed region the dominant kernel's launches are sampled (two event records per launch cost
                                 # a launch-bound step ~1.5 %); the single-stream replay behind it brackets every launch
SINGLE_STREAM_STEPS = 5
HEADLINE_MAX_BYTES = 3072        # the driver keeps the last ~8 KB of stdout and parses the last line: the headline line stays under 3 KB
DETAIL_FILE = "bench_detail.json"
DUMP_MAX_BYTES = 64 << 20        # --dump-outputs: all arrays together
DUMP_SAMPLE = 1 << 20            # elements kept of an array larger than its share of DUMP_MAX_BYTES (fixed, seeded sample)


def dump_outputs(outdir, arrays):
    """--dump-outputs: every array as `outdir/<name>.npy`, float64 for float64 data, float32 otherwise.  An array larger than its
    share of DUMP_MAX_BYTES is cut to a fixed, seeded sample of DUMP_SAMPLE elements of its flattened form (same indices every run)."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    share = DUMP_MAX_BYTES // max(1, len(arrays))
    total = 0
    for name, t in arrays.items():
        a = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(t)
        a = a.double() if a.dtype == torch.float64 else a.float()
        a = a.numpy()
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=min(DUMP_SAMPLE, share // a.itemsize), replace=False))
            a = a.reshape(-1)[idx]
        total += a.nbytes
        np.save(os.path.join(outdir, name + ".npy"), a)
    assert total <= DUMP_MAX_BYTES, total


def synthetic(n, h, w, seed, device):
    g = torch.Generator().manual_seed(seed)
    clean = torch.rand(n, 1, h, w, generator=g)
    label = torch.randint(0, 4, (n, h, w), generator=g)
    noisy = torch.clamp(clean + 0.05 * torch.randn(n, 1, h, w, generator=g), 0, 1)
    return clean.to(device), label.to(device), noisy.to(device), (clean, label, noisy)


def latent_mask_roofline(device):
    """The north-star's named kernel: score + rank-select + apply, channel mode, ONE launch (ctl_latent_mask_fused).  Algorithmic
    bytes = 3*N*C*h*w*4 (+ vectors).  Configured size (16x128x16x16, 2 MiB/tensor: cache-resident, launch-latency bound) and a
    128 MiB/tensor problem (HBM-bound).  Timed with events on torch's current stream, which is the stream the kernel is launched on."""
    from cooperative_training_and_latent_space_data_augmentation_amd import ops
    out = {}
    for tag, (n, c, h, w) in (("configured_16x128x16x16", (16, 128, 16, 16)), ("hbm_regime_64x128x64x64", (64, 128, 64, 64))):
        grad = torch.randn(n, c, h, w, device=device).contiguous(memory_format=torch.channels_last)
        code = torch.rand(n, c, h, w, device=device).contiguous(memory_format=torch.channels_last)
        for _ in range(3):
            ops.latent_mask(grad, code, 0, c // 3)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        iters = 20
        ev[0].record()
        for _ in range(iters):
            ops.latent_mask(grad, code, 0, c // 3)
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / iters
        nbytes = 12 * n * c * h * w + 8 * n * c
        out[tag] = {"bound": "hbm", "achieved": nbytes / us / 1e3, "peak": PEAK_HBM_GBS, "unit": "GB/s", "launches_per_call": 1,
                    "frac": nbytes / us / 1e3 / PEAK_HBM_GBS, "us_per_call": us, "algorithmic_mb": nbytes / 1e6}
        if n * c * h * w * 4 <= (8 << 20):
            # at this size the Python loop above measures the host's launch rate, not the kernel: replay the same launches from a
            # captured HIP graph (how the training step runs them in graph mode) to time the GPU side alone
            try:
                g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    ops.latent_mask(grad, code, 0, c // 3)          # the per-stream workspace must exist before capture
                    with torch.cuda.graph(g, stream=side):
                        for _ in range(10):
                            ops.latent_mask(grad, code, 0, c // 3)
                torch.cuda.current_stream().wait_stream(side)
                g.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                gus = e0.elapsed_time(e1) * 1e3 / 100
                out[tag].update({"graph_replay_us_per_call": gus, "graph_replay_gbs": nbytes / gus / 1e3,
                                 "graph_replay_frac": nbytes / gus / 1e3 / PEAK_HBM_GBS})
            except Exception as exc:                      # graph capture is an extra; the eager figure above stands on its own
                out[tag]["graph_replay_error"] = str(exc)[:120]
    return out


def cpu_baseline(host_batch, threads, steps=5, warm=3, cfgs=(DROP_IMG, DROP_SEG), what="dropout masks"):
    """BASELINE.md section 3 procedure: the full bs16 batch, `warm` warm-up steps + `steps` timed steps, median (the oracle is the checker,
    timed here as the reported CPU baseline -- never on the product path).  The headline run does 3 + 5; the
    sub-record children do 1 + 3 so that the default run stays within a few minutes (--cpu-baseline-steps)."""
    from oracle import ref_cpu as O
    from cooperative_training_and_latent_space_data_augmentation_amd.init import reference_init_state_dicts
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    s = O.OracleSolver(state_dicts=reference_init_state_dicts())
    clean, label, noisy = host_batch
    times = []
    for i in range(warm + steps):
        t0 = time.perf_counter()
        s.cooperative_step(clean, label, noisy, cfgs[0], cfgs[1])
        times.append(time.perf_counter() - t0)
    med = sorted(times[warm:])[len(times[warm:]) // 2]
    n, hw = clean.shape[0], clean.shape[-1]
    return {"value": n / med, "unit": "slices/s", "cores": threads, "kind": "port",
            "sample": f"oracle/ref_cpu.py, full cooperative step bs{n} {hw}x{hw} fp32, {threads} torch threads: {warm} warm-up + {steps} timed steps, median {med:.1f} s/step",
            "sample_detail": f"{what}; warm-up {[round(t, 1) for t in times[:warm]]} s, timed {[round(t, 1) for t in times[warm:]]} s; the reference's arithmetic"}


def cpu_baselines_other_configs(host_batch, threads):
    """BASELINE.md section 3 asks for CPU figures beside every config: configs[0] (bs4, standard_training step only: the reference's own
    CPU-runnable case), the config-4 masking scheme (all three schemes randomly sampled) and the swapped config-3 pair (spatial masks on the
    image code, channel masks on the shape code).  The oracle is the checker, timed here as the reported baseline; 1 warm-up + 3 timed steps
    each (the headline's configs[1] figure does 3 + 5)."""
    import random
    from oracle import ref_cpu as O
    from cooperative_training_and_latent_space_data_augmentation_amd.init import reference_init_state_dicts
    torch.set_num_threads(threads)
    clean, label, noisy = host_batch
    out = {}
    swapped = (dict(TGT_IMG, mask_type="spatial"), dict(TGT_SEG, mask_type="channel"))
    for tag, n, cfgs, latent_da, what in (("config0_bs4_standard_only", 4, (None, None), False, "standard_training + backward + 5x Adam, no latent-space augmentation"),
                                           ("config4_random_masks", clean.shape[0], (RND_IMG, RND_SEG), True, "full cooperative step, all three masking schemes randomly sampled"),
                                           ("config3_swapped_spatial_channel", clean.shape[0], swapped, True, "full cooperative step, spatial masks on the image code + channel masks on the shape code")):
        torch.manual_seed(0)
        random.seed(0)
        s = O.OracleSolver(state_dicts=reference_init_state_dicts())
        times = []
        for _ in range(4):
            t0 = time.perf_counter()
            s.cooperative_step(clean[:n], label[:n], noisy[:n], cfgs[0], cfgs[1], latent_DA=latent_da)
            times.append(time.perf_counter() - t0)
        med = sorted(times[1:])[1]
        out[tag] = {"value": n / med, "unit": "slices/s", "cores": threads, "kind": "port",
                    "sample": f"oracle/ref_cpu.py, {what}, bs{n} {clean.shape[-1]}x{clean.shape[-1]} fp32, {threads} torch threads: 1 warm-up + 3 timed steps, median {med:.2f} s/step"}
    return out


def _narrow(k):
    """1x1 convs, the <= 4-channel first layers (K-packed taps, in3) and the launches with fewer than 16 output channels (id suffix ,coN):
    8-32 flop per byte, HBM-side members of the conv families"""
    return "<ks1," in k or ",in3," in k or ",co" in k


# (the two conv families whole, as round 2 reported them, and split by what bounds their members: the 3x3 / 4x4 / 2x2 forms on >= 16
# channels are matrix work, the 1x1 convs and the first layers stream)
FAMILIES = (("conv_fwd_dgrad", lambda k: k.startswith("conv_igemm")), ("weight_gradients", lambda k: k.startswith("conv_wgrad")),
            ("conv_fwd_dgrad_3x3", lambda k: k.startswith("conv_igemm") and not _narrow(k)),
            ("conv_fwd_dgrad_1x1_and_first_layers", lambda k: k.startswith("conv_igemm") and _narrow(k)),
            ("weight_gradients_3x3", lambda k: k.startswith("conv_wgrad") and not _narrow(k)),
            ("weight_gradients_1x1_and_first_layers", lambda k: k.startswith("conv_wgrad") and _narrow(k)),
            ("batchnorm_backward", lambda k: k.startswith(("bwd_reduce<0>", "bwd_reduce<1>", "bwd_apply"))),
            ("other_hbm_passes", lambda k: k.startswith(("bn_act", "sumpool2", "bwd_reduce<2>"))))


def family_rooflines(prof, dtype, steps):
    """Per-family and per-kernel rooflines of ONE step from the single-stream replay (every launch bracketed with HIP events on its
    launch stream): conv families against the MFMA peak of the arithmetic type or HBM, whichever bounds them; the element-wise passes
    against HBM.  `ms_per_step` is serialised kernel time (the timed region overlaps two launch chains)."""
    out = {}
    for fam, member in FAMILIES:
        ids = {k: v for k, v in prof.items() if member(k)}
        if not ids:
            continue
        ms = sum(v["ms"] for v in ids.values())
        fl, by, n = sum(v["flops"] for v in ids.values()), sum(v["bytes"] for v in ids.values()), sum(v["launches"] for v in ids.values())
        tf, gbs = fl / ms / 1e9, by / ms / 1e6
        # matrix side: every member against the peak of ITS pipe (fp32 MFMA, or bf16 MFMA / 6 for the X3 launches), weighted by time
        f_m = sum(v["flops"] / 1e9 / peak_mfma_of(k, dtype) for k, v in ids.items()) / ms
        f_h = gbs / PEAK_HBM_GBS
        rec = {"bound": "mfma" if f_m >= f_h else "hbm", "frac": max(f_m, f_h), "tflops": tf, "hbm_gbs": gbs, "mfma_frac": f_m, "hbm_frac": f_h,
               "tflops_over_fp32_mfma_peak": tf / PEAK_MFMA_F32_TFLOPS if dtype != "bf16" else None,
               "launches_per_step": n / steps, "ms_per_step": ms / steps, "algorithmic_gflop_per_step": fl / steps / 1e9,
               "algorithmic_gb_per_step": by / steps / 1e9, "kernels": {}}
        for k, v in sorted(ids.items(), key=lambda kv: -kv[1]["ms"])[:6]:
            ktf, kgb = v["flops"] / v["ms"] / 1e9, v["bytes"] / v["ms"] / 1e6
            pk = peak_mfma_of(k, dtype)
            rec["kernels"][k] = {"launches_per_step": v["launches"] / steps, "avg_us": 1e3 * v["ms"] / v["launches"], "tflops": ktf, "hbm_gbs": kgb,
                                 "peak_tflops": pk, "frac": max(ktf / pk, kgb / PEAK_HBM_GBS), "bound": "mfma" if ktf / pk >= kgb / PEAK_HBM_GBS else "hbm"}
        out[fam] = rec
    return out


def sub_record(argv, tag):
    """Run this script in a child process (never an exec of this one: it holds the GPU) and return its full record: the child writes
    its detail file, the parent embeds it; the child's stdout line is its own (cut-down) headline."""
    dfile = f"bench_detail_{tag}.json"
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv + ["--detail-file", dfile], capture_output=True, text=True, timeout=900, cwd=ROOT)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": f"rc={r.returncode}: {r.stderr[-300:]}"}
        try:
            return json.load(open(os.path.join(ROOT, dfile)))
        except (OSError, ValueError):
            return json.loads(lines[-1])
    except Exception as exc:
        return {"error": f"{type(exc).__name__}: {str(exc)[:200]}"}


def inference_main(args, device):
    """BASELINE configs[4]: 3-D volume inference, 192x192xN stacks, FTN+STN forward only (model.py:375-394 through
    test_basic_segmentation_solver.py:85-114), eval-mode BatchNorm, argmax to a uint8 label volume.  Two forms of the same computation:
    the reference's chunks of <= 10 slices, and the whole volume in one pass (exact under eval-mode BatchNorm: slices are independent)."""
    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    slices, size, n_iter = 40, 192, 2
    g = torch.Generator().manual_seed(5)
    vol = torch.rand(slices, 1, size, size, generator=g)
    dvol = vol.to(device)
    gflop_per_slice = 4.14 * (size / 192.0) ** 2          # n_iter=2 with the redundant second STN pass removed (6.18 as the reference runs it)
    out = {"metric": "volume-inference slices/sec (192x192, n_iter=2, eval BatchNorm, argmax)", "unit": "slices/s", "n_gpus": 1, "dtype": "f32",
           "data": "synthetic", "higher_is_better": True,
           "config": {"workload": f"BASELINE configs[4]: {slices}-slice 192x192 volume, FTN + STN refinement (n_iter={n_iter}), uint8 label volume out; "
                                  "reference-init weights, non-trivial running statistics are not needed for timing"}}
    recs = {}
    # three calls of the same computation: the reference's arguments (chunk = 10; the engine runs the chunks as one pass, tester.COALESCE_CHUNKS:
    # exact under eval-mode BatchNorm), the reference's literal loop of 10-slice passes, and the whole volume asked for explicitly (--full:
    # a plain run times the first, the headline, alone)
    forms = (("reference_arguments_chunk10", 10, None), ("literal_chunk10_loop", 10, False), ("whole_volume", slices, None))
    for tag, chunk, coalesce in (forms if args.full else forms[:1]):
        fn = lambda: predict_volume(solver, dvol, n_iter=n_iter, chunk=chunk, coalesce=coalesce)
        for _ in range(max(2, args.warmup)):
            lab = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            lab = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        if tag == forms[0][0] and args.dump_outputs:
            dump_outputs(args.dump_outputs, {"label_volume": lab})
        assert lab.dtype == torch.uint8 and tuple(lab.shape) == (slices, size, size)
        recs[tag] = {"value": slices / dt, "ms_per_volume": 1e3 * dt, "chunk": chunk}
        if not args.full:
            continue
        _ffi.prof_start("")
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        prof = _ffi.prof_stop()
        fl = sum(v["flops"] for v in prof.values()) / 3
        kms = sum(v["ms"] for v in prof.values()) / 3
        kid, kr = max(prof.items(), key=lambda kv: kv[1]["ms"])
        ktf, kgb, pk = kr["flops"] / kr["ms"] / 1e9, kr["bytes"] / kr["ms"] / 1e6, peak_mfma_of(kid, "fp32")
        kbound = "mfma" if ktf / pk >= kgb / PEAK_HBM_GBS else "hbm"
        recs[tag].update({"roofline": {"kernel": kid, "bound": kbound, "achieved": ktf if kbound == "mfma" else kgb, "peak": pk if kbound == "mfma" else PEAK_HBM_GBS,
                                  "unit": "TFLOP/s" if kbound == "mfma" else "GB/s", "frac": max(ktf / pk, kgb / PEAK_HBM_GBS), "avg_us": 1e3 * kr["ms"] / kr["launches"],
                                  "launches": int(kr["launches"]), "traffic": None,
                                  "measured": "HIP events around every launch of this id in 3 passes behind the timed region; id = arg-max of serial kernel time"},
                     "whole_path": {"conv_tflops_over_wall_time": fl / dt / 1e12, "frac_of_fp32_mfma_peak": fl / dt / 1e12 / PEAK_MFMA_F32_TFLOPS,
                                    "executed_conv_gflop_per_slice": fl / slices / 1e9, "reference_gflop_per_slice": gflop_per_slice,
                                    "serial_conv_kernel_ms": kms},
                     "kernels_by_serial_time": [{"kernel": k, "ms_per_volume": v["ms"] / 3, "avg_us": 1e3 * v["ms"] / v["launches"],
                                                 "tflops": v["flops"] / v["ms"] / 1e9, "hbm_gbs": v["bytes"] / v["ms"] / 1e6}
                                                for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:8]]})
    head = recs["reference_arguments_chunk10"]
    out.update({"value": head["value"], "ms_per_step": head["ms_per_volume"], "steps": args.steps, "warmup": args.warmup, "forms": recs})
    if "roofline" in head:
        out["roofline"] = head["roofline"]
    if args.full and not args.no_cpu_baseline:
        from oracle import ref_cpu as O
        from cooperative_training_and_latent_space_data_augmentation_amd.init import reference_init_state_dicts
        threads = args.cpu_threads or min(32, os.cpu_count())
        torch.set_num_threads(threads)
        torch.manual_seed(0)
        o = O.OracleSolver(state_dicts=reference_init_state_dicts())
        o.eval()
        ts = []
        with torch.no_grad():
            for _ in range(4):
                t0 = time.perf_counter()
                for c0 in range(0, slices, 10):
                    o.predict(vol[c0:c0 + 10], n_iter=n_iter).argmax(1)
                ts.append(time.perf_counter() - t0)
        med = sorted(ts[1:])[1]
        out["cpu_baseline"] = {"value": slices / med, "unit": "slices/s", "cores": threads, "kind": "port",
                               "sample": f"oracle/ref_cpu.py predict(n_iter={n_iter})+argmax, {slices}-slice volume in chunks of 10, {threads} torch threads: "
                                         f"1 warm-up + 3 volumes, median {med:.2f} s"}
    emit(out, args)


def flush_c_stdio():
    """RCCL writes its version banner to C stdout while the first communicator is built; redirected to a file that buffer is only
    written at process exit -- BEHIND the JSON line.  Flushing it early keeps the JSON line the last line of the job's stdout."""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) without a launcher: this process touches no GPU (torch.cuda.device_count() does not initialise
    one on this image), starts the N ranks as a CHILD process -- python -m torch.distributed.run, one rank per GPU, rendezvous on
    127.0.0.1 -- relays the job's stdout (rank 0's headline line last) and exits with the job's code.  Fewer than N visible devices is
    an error, never a silent smaller run."""
    import socket
    n_dev = torch.cuda.device_count()
    if n_dev < 1 or (n_dev < args.gpus and not args.all_on_device0):
        print(f"bench.py: --gpus {args.gpus} but {n_dev} GPU(s) visible: refusing to run a smaller job under that label", file=sys.stderr)
        return 2
    with socket.socket() as sk:                           # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)
    lines = r.stdout.splitlines()
    head = [l for l in lines if l.startswith("{")]
    for l in lines:                                       # everything the job printed, then rank 0's headline line as the LAST line
        if not head or l is not head[-1]:
            print(l)
    if r.returncode == 0 and not head:
        print("bench.py: the launched job printed no headline line", file=sys.stderr)
        return 3
    if head:
        rec = json.loads(head[-1])
        if r.returncode == 0 and rec.get("n_gpus") != args.gpus:
            print(f"bench.py: asked for {args.gpus} ranks, the job reports n_gpus = {rec.get('n_gpus')}", file=sys.stderr)
            return 4
        flush_c_stdio()
        print(head[-1], flush=True)
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--mode", default="auto", choices=["auto", "eager", "graph", "segments"],
                    help="eager: Python issues the ~900 launches of a step on two HIP streams; graph: the whole step is one hipGraph replay "
                         "(host-insensitive); segments: the captured step replayed as linear per-chain segment graphs on two streams "
                         "(hipgraph.SegmentReplay, also host-insensitive); auto: all three are timed for a few untimed steps after the warm-up "
                         "and the fastest one is measured")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                    help="fp32: the reference's arithmetic (BASELINE configs[1], the headline; nets.X3: the 3x3 / 4x4 / 2x2 contractions run on the bf16 "
                         "matrix pipe over an exact three-way split of the fp32 operands, same results class as fp32 MFMA); bf16: configs[2] -- network-internal "
                         "activations / gradients stored as bf16, convolutions on v_mfma_f32_16x16x32_bf16, fp32 accumulate / BatchNorm "
                         "statistics / master weights / losses")
    ap.add_argument("--masks", default=None, choices=list(MASKS), help="latent masking scheme (default: dropout for fp32, targeted for bf16)")
    ap.add_argument("--workload", default="step", choices=["step", "inference"],
                    help="step: the cooperative-training iteration (headline); inference: BASELINE configs[4], 192x192 volume inference")
    ap.add_argument("--no-sub-records", action="store_true", help="headline only (the sub-records are measured by child processes)")
    ap.add_argument("--lib", default=None, help="A/B aid: path of another build of libctl_hip.so (tools/ab.sh)")
    ap.add_argument("--set", action="append", default=[], metavar="MODULE.ATTR=VALUE",
                    help="A/B aid: set a plan-compiler switch before the solver is built, e.g. nets.FUSE_BNBWD=True")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--single-stream", action="store_true", help="A/B aid: one launch chain instead of two (solver.two_streams = False)")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--cpu-baseline-steps", default="3+5", help="warm-up + timed steps of the CPU baseline (BASELINE.md section 3: >= 3 + >= 5)")
    ap.add_argument("--prof-filter", default=None, help="profiling id to report as `roofline.kernel` instead of the arg-max of serial time")
    ap.add_argument("--detail-file", default=DETAIL_FILE, help="where the full record goes (relative to this script)")
    ap.add_argument("--detail-to-stdout", action="store_true", help="also print the BENCH_DETAIL line to stdout (before the headline line)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed (RCCL) even for a world of 1")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl == RCCL; gloo only for control-flow tests)")
    ap.add_argument("--all-on-device0", action="store_true", help="test aid: every rank uses GPU 0 (needs --backend gloo)")
    ap.add_argument("--check-finite", action="store_true", help="debug aid: synchronise and check losses / weights / gradients / buffers after every step of every phase")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: the dominant kernel's roofline (single-stream profiles before and "
                         "behind the timed region, sampled events inside it in eager mode), per-family rooflines, the launch census, the "
                         "latent-mask roofline, the CPU baselines and, at N=1, the sub-records of the other configs (child processes)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path computed in its last timed step to DIR/<name>.npy (float32 / float64, <= 64 MB in all)")
    args = ap.parse_args()

    if args.masks is None:
        args.masks = "targeted" if args.dtype == "bf16" else "dropout"
    IMG_CFG, SEG_CFG, mask_text = MASKS[args.masks]
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))              # (before anything in this process touches a GPU)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback of the product path)")
    if args.all_on_device0:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    import torch.distributed as dist
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend=args.backend, rank=rank, world_size=world)

    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
    if args.lib:
        _ffi.LIB_PATH = os.path.abspath(args.lib)
    import importlib
    for kv in args.set:
        target, val = kv.split("=", 1)
        modname, attr = target.rsplit(".", 1)
        setattr(importlib.import_module("cooperative_training_and_latent_space_data_augmentation_amd." + modname), attr, eval(val))
    if args.workload == "inference":
        return inference_main(args, device)
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.dist import DataParallel

    import random
    import numpy as np
    torch.manual_seed(0)                                 # identical initial weights on every rank
    random.seed(0)                                       # (the host draws of the masking schemes: identical inputs from run to run)
    np.random.seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4,
                                                   learning_rate=1e-4, use_gpu=True, compute_dtype=args.dtype)
    if args.single_stream:
        solver.two_streams = False
    dp = DataParallel(solver) if use_dist else None
    if use_dist:
        flush_c_stdio()                                   # (the weight broadcast built the communicator: its banner goes out now)
    if use_dist:                                         # per-rank RNG streams (scheme / k / dropout / soft-noise draws), after the weight broadcast
        torch.manual_seed(1234 + rank)
        np.random.seed(1234 + rank)
        random.seed(1234 + rank)
    clean, label, noisy, host_batch = synthetic(args.batch, args.size, args.size, 1000 + rank, device)
    # eager steps: every network's range of the gradient bucket is all-reduced from inside the backward sweep as soon as that network's
    # last backward pass has been issued, and its Adam launch waits for that range only (dist.py); graph mode: the five exchanges run
    # between the forward/backward graph and the Adam graph
    hook = dp.launch_remaining if dp else None
    hook_graph = dp.sync_gradients if dp else None

    check_state = {"calls": 0, "bad": None}

    def check_finite(what, losses):
        """--check-finite (debug aid, tools/debug/r6_dp_flake.sh): after EVERY step of every phase, name the first non-finite loss / weight /
        gradient / BatchNorm buffer (a NaN otherwise only shows in the final losses, many steps and phases later)."""
        check_state["calls"] += 1
        if not args.check_finite or check_state["bad"]:
            return losses
        torch.cuda.synchronize()
        bad = []
        if not all(bool(torch.isfinite(v)) for v in losses):
            bad.append("losses")
        for k, m in solver.model.items():
            for tag, t in (("weights", m._flat_data), ("gradient", m._flat.grad), ("bn_buffers", m._bflat)):
                if not bool(torch.isfinite(t).all()):
                    bad.append(f"{tag}:{k}")
        if bad:
            check_state["bad"] = f"rank {rank} call {check_state['calls']} ({what}, two_streams={solver.two_streams}): {bad}"
            print("CHECK_FINITE " + check_state["bad"], file=sys.stderr, flush=True)
        return losses

    def eager_step():
        return check_finite("eager", solver.cooperative_step(clean, label, noisy, IMG_CFG, SEG_CFG, grad_hook=hook))

    step = eager_step

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()

    def single_stream_profile(nsteps):
        """The step replayed on ONE stream with every conv-family launch and every HBM-bound plan op bracketed by HIP events on its
        launch stream, each with its algorithmic work (rank 0 profiles; EVERY rank replays: step() contains the gradient all-reduce).
        In the timed region two launch chains share the GPU, so a kernel's event-timed duration there includes the time it shares
        the CUs with the other chain; this replay is the kernel-quality figure and what rocprofv3 --kernel-trace (which serialises
        dispatches) shows."""
        two = getattr(solver, "two_streams", False)
        solver.two_streams = False
        try:
            for _ in range(2):
                eager_step()
            torch.cuda.synchronize()
            if rank == 0:
                _ffi.prof_start("")
            for _ in range(nsteps):
                eager_step()
            torch.cuda.synchronize()
            return _ffi.prof_stop() if rank == 0 else {}
        finally:
            solver.two_streams = two

    # which kernel is `roofline.kernel`: the arg-max of serial time over the profiling ids of one step (still untimed)
    # (--full only: a plain run records no per-launch events anywhere)
    dominant = user_filter = args.prof_filter
    if args.full and rank == 0 and dominant is None:
        pre = single_stream_profile(2)
        dominant = max(pre.items(), key=lambda kv: kv[1]["ms"])[0] if pre else ""
    elif args.full and dominant is None:
        single_stream_profile(2)
        dominant = ""
    args.prof_filter = dominant
    sample_dominant = args.full and rank == 0
    fence()
    # ---- execution mode (still untimed): the step as a hipGraph replay vs Python-issued launches
    from cooperative_training_and_latent_space_data_augmentation_amd.graph import CooperativeStepGraph
    calib, mode, gstep = {}, args.mode, None
    if mode in ("auto", "graph", "segments"):
        try:
            gstep = CooperativeStepGraph(solver, IMG_CFG, SEG_CFG, grad_hook=hook_graph, replay="segments" if mode == "segments" else "runtime")
            graph_step = lambda: check_finite("graph:" + gstep.replay_mode, gstep(clean, label, noisy))
            graph_step()                                  # capture + first replay
            if args.masks == "random":                    # one captured graph per (image scheme, shape scheme) pair: capture all nine BEFORE the timed
                for _ in range(200):                      # region (the scheme is drawn per step: a first-time pair inside it would time a capture)
                    done = torch.tensor([1.0 if len(gstep.entries) >= 9 else 0.0], device=device)
                    if use_dist:                          # each rank draws its own schemes but every step carries the gradient exchange:
                        dist.all_reduce(done, op=dist.ReduceOp.MIN)   # all ranks run the same number of steps
                    if done.item() > 0:
                        break
                    graph_step()
                calib["scheme_pair_graphs"] = len(gstep.entries)
            fence()
        except Exception as exc:                          # capture is an optimisation: the eager path is the same computation
            if mode in ("graph", "segments"):
                raise
            calib["graph_error"], gstep = f"{type(exc).__name__}: {str(exc)[:160]}", None
    if use_dist and mode == "auto":                       #  every later collective is reached by all ranks or by none: a rank
        cap_ok = torch.tensor([1.0 if gstep is not None else 0.0], device=device)   # whose capture failed takes the others to the eager step too
        dist.all_reduce(cap_ok, op=dist.ReduceOp.MIN)
        if cap_ok.item() == 0 and gstep is not None:
            calib["graph_error"], gstep = "capture failed on another rank", None
    if mode == "auto":
        def time_steps(fn, n=8):
            fence()
            t = time.perf_counter()
            for _ in range(n):
                fn()
            fence()
            return 1e3 * (time.perf_counter() - t) / n
        if sample_dominant:                               # as in the timed region: eager steps carry the per-launch events of the
            _ffi.prof_start(args.prof_filter, PROF_EVERY) # dominant kernel (the roofline figure), graph replays cannot
        calib["eager_ms"] = time_steps(eager_step)
        if sample_dominant:
            _ffi.prof_stop()
        if gstep is not None:
            calib["graph_ms"] = time_steps(graph_step)
            seg_ok = 1.0
            try:                                          # the same captured graphs as linear segment graphs on two streams
                gstep.set_replay_mode("segments")
            except Exception as exc:
                seg_ok, calib["segments_error"] = 0.0, f"{type(exc).__name__}: {str(exc)[:160]}"
            flag = torch.tensor([seg_ok], device=device)
            if use_dist:                                  # (every timed step carries the gradient exchange: all ranks time it, or none)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if flag.item() > 0:
                graph_step()                              # (untimed: the first segment replay probes the hardware queues of its streams)
                calib["segments_ms"] = time_steps(graph_step)
                calib["segments"] = next(iter(gstep.entries.values())).segments.describe()
            else:
                gstep.set_replay_mode("runtime")
        best = min((calib.get(k + "_ms", float("inf")), i) for i, k in enumerate(("eager", "graph", "segments")))[1]
        pick = torch.tensor([float(best)], device=device)
        if use_dist:                                      # every rank must run the same mode: rank 0 decides
            dist.broadcast(pick, 0)
        mode = ("eager", "graph", "segments")[int(pick.item())]
        if gstep is not None:
            gstep.set_replay_mode("segments" if mode == "segments" else "runtime")
    if mode in ("graph", "segments"):
        step = graph_step
    elif gstep is not None:                               # eager chosen: give the graph's private pool back and let the allocator settle
        del gstep, graph_step
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        # as many un-synchronised steps as the timed region has: the host runs several steps ahead of the GPU there, blocks that carry
        # a record_stream() mark are reused late, and the pool only stops growing once it has seen that depth (3 steps: 14 device
        # allocations and one 13.5-ms step inside the timed region)
        for _ in range(max(8, args.steps)):
            eager_step()
        fence()
    # launches of one step: the library's own census over one eager step (untimed; the graph replays the same launches as nodes) +
    # what ATen adds (fills / copies / cats: counted by the profiler once in tools/aten_ops_in_step.py, ~45 per step, not re-counted here)
    launches_per_step = None
    if args.full:
        n0 = _ffi.lib.ctl_launch_count()
        eager_step()
        fence()
        launches_per_step = int(_ffi.lib.ctl_launch_count() - n0)
    phase_tm = None
    if rank == 0 and args.lib and hasattr(_ffi.lib, "ctl_debug_timing"):
        import ctypes                                     # -DCTL_TIMING variant build: per-phase cycle counters of the conv kernel
        phase_tm = (ctypes.c_ulonglong * 12)()
        _ffi.lib.ctl_debug_timing(phase_tm)               # reset
    if sample_dominant and mode == "eager":               # per-launch HIP events cannot be recorded inside a graph replay
        _ffi.prof_start(args.prof_filter, PROF_EVERY)     # (every 4th launch of the dominant kernel: ~250 samples in 20 steps)
    # per-step record: one event per step on the launch stream (no sync inside the timed region), the host's
    # issue time per step, and the caching allocator's device-allocation counter (a hipMalloc inside the region = a one-off stall)
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    issue_s = []
    alloc0 = torch.cuda.memory_stats().get("num_device_alloc", 0)
    alloc_at = []
    t0 = time.perf_counter()
    step_ev[0].record()
    for i in range(args.steps):
        ti = time.perf_counter()
        losses = step()
        issue_s.append(time.perf_counter() - ti)
        step_ev[i + 1].record()
        alloc_at.append(torch.cuda.memory_stats().get("num_device_alloc", 0))
    fence()
    dt = time.perf_counter() - t0
    step_ms = sorted(step_ev[i].elapsed_time(step_ev[i + 1]) for i in range(args.steps))
    allocs_in_region = torch.cuda.memory_stats().get("num_device_alloc", 0) - alloc0
    prof = _ffi.prof_stop() if (sample_dominant and mode == "eager") else {}
    if args.dump_outputs and rank == 0:                  # (before anything behind the timed region steps the solver again)
        arrays = {"losses": torch.stack([v.detach().double() for v in losses])}
        arrays.update({f"mask_{k}": m for k, m in sorted(solver.last_masks.items()) if m is not None})
        for k, m in solver.model.items():
            arrays[f"weights_{k}"] = m._flat_data
            arrays[f"bn_buffers_{k}"] = m._bflat
        dump_outputs(args.dump_outputs, arrays)
    # kernel-quality figures: the same step on ONE stream behind the timed region (see single_stream_profile)
    prof_all = single_stream_profile(SINGLE_STREAM_STEPS) if args.full else {}
    if user_filter:                                      # --prof-filter: report that id (exact, else substring match)
        prof_single = {k: v for k, v in prof_all.items() if k == user_filter} or {k: v for k, v in prof_all.items() if user_filter in k}
    else:                                                # the arg-max of THIS profile (the pre-region pick only chose what to sample in-region)
        prof_single = dict([max(prof_all.items(), key=lambda kv: kv[1]["ms"])]) if prof_all else {}
    if phase_tm is not None:
        _ffi.lib.ctl_debug_timing(phase_tm)
        steps = max(phase_tm[6], 1)
        names = ["issue", "mfma", "bar_rd", "stage", "bar_wr", "epi"]
        print("conv phase cycles per (tile, chunk) step per wave:", {k: round(phase_tm[i] / steps) for i, k in enumerate(names)},
              "setup/step", round(phase_tm[7] / steps), "MHz", round(100.0 * phase_tm[8] / max(phase_tm[9], 1)), file=sys.stderr)
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    loss_vals = [float(v) for v in losses]
    assert all(v == v and abs(v) < 1e6 for v in loss_vals), loss_vals

    from cooperative_training_and_latent_space_data_augmentation_amd import nets as _nets
    x3_on = args.dtype == "fp32" and bool(_nets.X3)
    if rank == 0:
        out = {
            "metric": "cooperative-training slices/sec (256x256, bs16 per GPU)", "value": world * args.batch * args.steps / dt,
            "unit": "slices/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16" if args.dtype == "bf16" else ("f32 (bf16x3 split)" if x3_on else "f32"), "data": "synthetic",
            "config": {"workload": f"ACDC-shaped synthetic {args.size}x{args.size}x1, batch {args.batch}/GPU, full cooperative step "
                                   f"(FTN+STN standard + {mask_text} + hard-example training + backward + 5x Adam), "
                                   "reference-init weights" + ("; bf16 storage of network-internal tensors + bf16 MFMA, fp32 accumulate / "
                                   "statistics / master weights (BASELINE configs[2])" if args.dtype == "bf16" else "") +
                                  ("; fp32 tensors and results, the 3x3/4x4/2x2 contractions on the bf16 matrix pipe over an exact 3-way split of the fp32 operands" if x3_on else ""),
                       "global_batch": world * args.batch,
                       "parallelism": f"dp{world}" if world > 1 else "single GPU"},
            "final_losses": loss_vals, "mode": mode, "mode_calibration": calib,
            "step_ms": {"min": step_ms[0], "median": step_ms[len(step_ms) // 2], "max": step_ms[-1],
                        "note": "GPU time between consecutive per-step events on the launch stream (rank 0)"},
            "cpu_issue_ms": {"median": 1e3 * sorted(issue_s)[len(issue_s) // 2], "max": 1e3 * max(issue_s)},
            "device_allocs_in_timed_region": int(allocs_in_region),
            "device_allocs_by_step": [int(b - a) for a, b in zip([alloc0] + alloc_at[:-1], alloc_at)],
            "chain_overlap": getattr(solver, "chain_overlap", None),
        }
        if launches_per_step is not None:
            out["launches_per_step"] = {"library": launches_per_step, "note": "kernels + stream memsets / copies enqueued by libctl_hip.so in one step "
                                        "(ctl_launch_count); PyTorch adds ~45 fills / copies per step (tools/aten_ops_in_step.py)"}
        def roofline_of(kid, rec, region_s=None, sampled_every=1):
            secs = rec["ms"] * 1e-3
            tf, gbs = rec["flops"] / secs / 1e12, rec["bytes"] / secs / 1e9
            peak_mfma = peak_mfma_of(kid, args.dtype)
            f_mfma, f_hbm = tf / peak_mfma, gbs / PEAK_HBM_GBS
            bound = "mfma" if f_mfma >= f_hbm else "hbm"
            r = {"bound": bound, "achieved": tf if bound == "mfma" else gbs,
                 "peak": peak_mfma if bound == "mfma" else PEAK_HBM_GBS,
                 "unit": "TFLOP/s" if bound == "mfma" else "GB/s", "frac": max(f_mfma, f_hbm), "traffic": None,
                 "kernel": kid, "launches": int(rec["launches"]), "avg_us": 1e3 * rec["ms"] / rec["launches"],
                 "algorithmic_gflop_per_launch": rec["flops"] / rec["launches"] / 1e9,
                 "algorithmic_mb_per_launch": rec["bytes"] / rec["launches"] / 1e6, "hbm_gbs": gbs, "hbm_frac": f_hbm, "tflops": tf}
            if peak_mfma not in (PEAK_MFMA_BF16_TFLOPS, PEAK_MFMA_F32_TFLOPS):
                r["peak_note"] = (f"X3 launch: fp32 operands split exactly into three bf16 numbers, {X3_PRODUCTS} bf16 MFMA products per fp32 product; peak = "
                                  f"{PEAK_MFMA_BF16_TFLOPS:.0f} / {X3_PRODUCTS} TFLOP/s algorithmic ({tf / PEAK_MFMA_F32_TFLOPS:.2f} of the 157.3 TFLOP/s fp32-MFMA peak)")
            if sampled_every > 1:                          # (the sampled count is not the launch count)
                r["sampled_every"] = sampled_every
                r["launches_note"] = f"every {sampled_every}-th launch was bracketed: `launches` counts the samples"
            elif region_s:
                r["share_of_serial_kernel_time"] = secs / region_s
            return r

        # `roofline`: the profiling id with the largest serial time, from the single-stream replay behind the timed region (HIP events
        # around EVERY launch on its launch stream; rocprofv3 --kernel-trace serialises dispatches and agrees with this duration).  In
        # eager mode the same kernel is also sampled INSIDE the timed region (`timed_region`: there it shares the CUs with the other chain).
        if prof_single:
            kid, rec = max(prof_single.items(), key=lambda kv: kv[1]["ms"])
            out["roofline"] = roofline_of(kid, rec, sum(v["ms"] for v in prof_all.values()) * 1e-3)
            out["roofline"]["measured"] = (f"HIP events around every launch of this id in {SINGLE_STREAM_STEPS} single-stream steps right behind the timed "
                                           "region (same process, same inputs); id = arg-max of serial kernel time over the step's profiling ids")
            if kid in prof:
                r1 = roofline_of(kid, prof[kid], None, PROF_EVERY)
                out["roofline"]["timed_region"] = {k: r1[k] for k in ("achieved", "frac", "avg_us", "launches", "sampled_every")}
        tfile = os.path.join(ROOT, "profiles", "kernel_traffic.json")      # committed rocprofv3 --pmc measurement, keyed by profiling id
        if "roofline" in out and os.path.exists(tfile):
            t = json.load(open(tfile)).get(args.dtype, {})
            if out["roofline"]["kernel"] in t.get("kernels", {}):
                out["roofline"]["traffic"] = t["kernels"][out["roofline"]["kernel"]]["hbm_bytes_per_launch"]
                out["roofline"]["traffic_source"] = t["kernels"][out["roofline"]["kernel"]].get("source") or t.get("source", "profiles/kernel_traffic.json")
        # the WHOLE step against its floor (VERDICT r5 "next" #7: `roofline` above describes one kernel, a few per cent of the time): ideal-fusion
        # HBM bytes of the step at 8 TB/s, next to the matrix-side floor of its algorithmic flops on the pipe the contractions run on
        gb = STEP_GB_PER_SLICE[args.masks] * args.batch * (0.5 if args.dtype == "bf16" else 1.0) * (args.size / 256.0) ** 2
        tflop = STEP_GFLOP_PER_SLICE[args.masks] * args.batch * (args.size / 256.0) ** 2 / 1e3
        pipe = PEAK_MFMA_BF16_TFLOPS if args.dtype == "bf16" else (PEAK_MFMA_BF16_TFLOPS / X3_PRODUCTS if x3_on else PEAK_MFMA_F32_TFLOPS)
        hbm_ms, mfma_ms = gb / PEAK_HBM_GBS * 1e3, tflop / pipe * 1e3
        floor = max(hbm_ms, mfma_ms)
        out["roofline_step"] = {"bound": "hbm" if hbm_ms >= mfma_ms else "mfma", "floor_ms": floor, "frac": floor / out["ms_per_step"],
                                "ideal_hbm_gb": gb, "hbm_floor_ms": hbm_ms, "algorithmic_tflop": tflop, "matrix_floor_ms": mfma_ms, "matrix_peak_tflops": pipe,
                                "note": "per rank; ideal fusion = every conv reads its input once and writes its output once (SURVEY 8(d))"}
        if prof_all:
            out["roofline_families"] = family_rooflines(prof_all, args.dtype, SINGLE_STREAM_STEPS)
            out["kernels_by_serial_time"] = [{"kernel": k, "ms_per_step": v["ms"] / SINGLE_STREAM_STEPS, "launches_per_step": v["launches"] / SINGLE_STREAM_STEPS,
                                              "avg_us": 1e3 * v["ms"] / v["launches"]}
                                             for k, v in sorted(prof_all.items(), key=lambda kv: -kv[1]["ms"])[:16]]
        if world == 1 and args.full:
            out["roofline_latent_mask"] = latent_mask_roofline(device)
        if world == 1 and args.full and not args.no_cpu_baseline:
            cb_warm, cb_steps = (int(v) for v in args.cpu_baseline_steps.split("+"))
            out["cpu_baseline"] = cpu_baseline(host_batch, args.cpu_threads or min(32, os.cpu_count()), steps=cb_steps, warm=cb_warm, cfgs=(IMG_CFG, SEG_CFG), what=mask_text)
        if world == 1 and args.full and not args.no_cpu_baseline and not args.no_sub_records and args.dtype == "fp32" and args.masks == "dropout":
            out["cpu_baselines_other_configs"] = cpu_baselines_other_configs(host_batch, args.cpu_threads or min(32, os.cpu_count()))
        if world == 1 and args.full and not args.no_sub_records and args.dtype == "fp32" and args.masks == "dropout":
            # BASELINE configs[2] and configs[4], each measured by a child process running this script (a fresh process: its own
            # streams, pools and graphs; this process is idle meanwhile).  The headline keys above are untouched.
            common = ["--full", "--steps", str(args.steps), "--warmup", str(args.warmup), "--no-sub-records", "--cpu-baseline-steps", "1+3"] + \
                     (["--no-cpu-baseline"] if args.no_cpu_baseline else []) + \
                     (["--lib", args.lib] if args.lib else []) + [x for kv in args.set for x in ("--set", kv)]
            # the control next to the X3 headline: the same step with every contraction on the fp32 matrix pipe
            # (v_mfma_f32_16x16x4_f32), i.e. nets.X3 = nets.X3_WGRAD = False
            if x3_on:
                out["config2_fp32_mfma"] = sub_record(["--set", "nets.X3=False", "--set", "nets.X3_WGRAD=False", "--no-cpu-baseline"] +
                                                      [a for a in common if a != "--no-cpu-baseline"], "config2_fp32_mfma")
            out["config3_bf16"] = sub_record(["--dtype", "bf16", "--masks", "targeted"] + common, "config3_bf16")
            out["config5_inference"] = sub_record(["--workload", "inference"] + common, "config5_inference")
            # BASELINE configs[3]'s masking scheme (all three schemes randomly sampled per step: one captured graph per scheme pair) at N = 1 --
            # the 8-GPU run itself is the driver's; this is the per-GPU step it scales from
            out["config4_random_masks_n1"] = sub_record(["--masks", "random", "--mode", "graph", "--no-cpu-baseline"] + [a for a in common if a != "--no-cpu-baseline"],
                                                        "config4_random_masks_n1")
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        emit(out, args)


def emit(detail, args):
    """bench_detail.json + the BENCH_DETAIL line (stderr), then the headline line: the LAST thing this job writes to stdout."""
    detail["detail_file"] = args.detail_file
    line = json.dumps(headline(detail))
    assert len(line) < HEADLINE_MAX_BYTES, len(line)
    blob = json.dumps(detail)
    try:
        with open(os.path.join(ROOT, args.detail_file), "w") as f:
            f.write(blob + "\n")
    except OSError as exc:                                # a read-only checkout must not cost the run its headline
        print(f"bench.py: could not write {args.detail_file}: {exc}", file=sys.stderr)
    print("BENCH_DETAIL " + blob, file=sys.stderr, flush=True)
    flush_c_stdio()
    if args.detail_to_stdout:
        print("BENCH_DETAIL " + blob, flush=True)
    print(line, flush=True)


def _sub_headline(rec):
    if not isinstance(rec, dict) or "value" not in rec:
        return {"error": str((rec or {}).get("error", "no record"))[:120]}
    return {"value": rec.get("value"), "ms_per_step": rec.get("ms_per_step"), "dtype": rec.get("dtype"), "mode": rec.get("mode"),
            "roofline_frac": (rec.get("roofline") or {}).get("frac"), "roofline_kernel": (rec.get("roofline") or {}).get("kernel"),
            "cpu_baseline_value": (rec.get("cpu_baseline") or {}).get("value")}


def headline(d):
    """The driver's line: contract keys + roofline + cpu_baseline + the two sub-records cut down; nothing that grows with the workload."""
    h = {k: d.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                               "vs_baseline", "dtype", "data")}
    c = d.get("config", {})
    h["config"] = {"workload": str(c.get("workload", ""))[:420], **{k: c[k] for k in ("global_batch", "parallelism") if k in c}}
    if "mode" in d:
        h["mode"] = d["mode"]
    r = d.get("roofline")
    if r:
        h["roofline"] = {k: r.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_us", "launches", "traffic") }
        if r.get("traffic_source"):
            h["roofline"]["traffic_source"] = str(r["traffic_source"])[:160]
    rs = d.get("roofline_step")
    if rs:
        h["roofline_step"] = {k: rs.get(k) for k in ("bound", "floor_ms", "frac")}
    cb = d.get("cpu_baseline")
    if cb:
        h["cpu_baseline"] = {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                             "sample": str(cb.get("sample", ""))[:160]}
    lm = (d.get("roofline_latent_mask") or {})
    if lm:
        h["latent_mask_hbm_frac"] = {k.split("_")[0] + "_" + k.split("_")[-1]: (v.get("graph_replay_frac") or v.get("frac")) for k, v in lm.items()}
    for k in ("config2_fp32_mfma", "config3_bf16", "config5_inference", "config4_random_masks_n1"):
        if k in d:
            h[k] = _sub_headline(d[k])
    h["detail"] = d.get("detail_file", DETAIL_FILE)
    return h


if __name__ == "__main__":
    main()
