"""One training batch from the device-resident set (loader.DeviceBatchLoader) against the numpy statement plus upload, next to the step
it feeds.

A synthetic training set of 20 volumes of 10 slices with in-plane sizes between 200 and 256 (pad 224 x 224, crop 192 x 192, default
canvas), batch size 16 with the original pair (8 slices drawn per batch), policy ACDC_affine_elastic_intensity:
  gather          ops.batch_gather alone (canvas batch and original pair, one launch): HIP events around one call, warm, median
                  ("eager"), and the same call captured into a graph and replayed ("graph")
  assemble        gather + augmenter (DeviceBatchLoader.assemble), eager and as a graph replay
  next_batch      the loader as a user calls it: epoch order, parameter draw, pinned copies, launches; wall time
  host            loader.gather_host for the same indices plus the upload of its four arrays, wall time on the same machine (upstream does
                  this per slice in DataLoader workers, with the augmentation on the host on top)
  step            one solver.cooperative_step on a batch of the same size, and assemble as a share of it
Nothing is asserted about the times.  Writes profiles/loader_batch.json.

    python tools/bench_loader.py [--out profiles/loader_batch.json] [--host-reps 5] [--device-reps 30]
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
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, basic_operations, loader as L  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter  # noqa: E402

PAD, CROP, BATCH, POLICY = (224, 224), (192, 192), 16, "ACDC_affine_elastic_intensity"
IMG_CFG = {"loss_name": "mse", "mask_type": "channel", "max_threshold": 0.5, "random_threshold": False, "if_soft": False}
SEG_CFG = {"loss_name": "ce", "mask_type": "spatial", "max_threshold": 0.5, "random_threshold": False, "if_soft": False}


def volumes(count=20, slices=10):
    rng = np.random.default_rng(0)
    out = []
    for _ in range(count):
        h, w = int(rng.integers(200, 257)), int(rng.integers(200, 257))
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        r = np.sqrt((yy - h / 2) ** 2 + (xx - w / 2) ** 2)
        label = np.zeros((slices, h, w), dtype=np.uint8)
        for k, radius in ((1, 40), (2, 28), (3, 14)):
            label[:, r < radius] = k
        image = (0.2 * label + 0.3 * rng.uniform(0, 1, (slices, h, w))).astype(np.float32)
        out.append((image, label))
    return out


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader_batch.json"))
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--device-reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    torch.manual_seed(0)
    vols = volumes()
    s = L.DeviceSliceSet(vols, PAD, CROP, device="cuda")
    host_slices = [(im[i], la[i]) for im, la in vols for i in range(im.shape[0])]
    loader = L.DeviceBatchLoader(s, BATCH, augmenter=BatchAugmenter(POLICY, CROP, seed=0), generator=torch.Generator().manual_seed(0))
    n = loader.train_batch_size
    index = np.random.default_rng(1).integers(0, len(s), n)
    index_dev = torch.from_numpy(index.astype(np.int32)).cuda()
    params = BatchAugmenter.upload(loader.augmenter.draw(n, *s.canvas), "cuda")
    out = loader.empty_batch(n)
    canvas = loader.canvas_buffers(n)

    def gather():
        s.gather(index_dev, with_orig=True, out=canvas, orig_out=(out[0][n:], out[1][n:]))

    def assemble():
        loader.assemble(index_dev, params, out)

    def host():
        return [torch.from_numpy(a).pin_memory().cuda(non_blocking=True) for a in L.gather_host(host_slices, index, s.lut_host, s.canvas, CROP)]

    rec = {"volumes": len(vols), "slices": len(s), "canvas": list(s.canvas), "crop": list(CROP), "batch_size": BATCH, "slices_per_batch": n,
           "policy": POLICY}
    for name, fn in (("gather", gather), ("assemble", assemble)):
        before = _ffi.lib.ctl_launch_count()
        fn()
        rec[f"{name}_kernel_launches"] = int(_ffi.lib.ctl_launch_count() - before)
        t, lo, hi = device_ms(fn, args.device_reps)
        rec[f"{name}_eager_ms"], rec[f"{name}_eager_ms_min_max"] = t, [lo, hi]
        eager = [o.clone() for o in out]
        graph = graph_of(fn)
        t, lo, hi = device_ms(graph.replay, args.device_reps)
        rec[f"{name}_graph_replay_ms"], rec[f"{name}_graph_replay_ms_min_max"] = t, [lo, hi]
        rec[f"{name}_graph_replay_bits_equal_eager"] = bool(torch.equal(out[0].view(torch.int32), eager[0].view(torch.int32))
                                                           and torch.equal(out[1], eager[1]))
        del graph
    _, t, lo, hi = timed(loader.next_batch, args.device_reps, 3)
    rec["next_batch_wall_ms"], rec["next_batch_wall_ms_min_max"] = t * 1e3, [lo * 1e3, hi * 1e3]
    got, t, lo, hi = timed(host, args.host_reps, 1)
    rec["host_gather_plus_upload_wall_ms"], rec["host_gather_plus_upload_wall_ms_min_max"] = t * 1e3, [lo * 1e3, hi * 1e3]
    gather()
    torch.cuda.synchronize()
    rec["gather_bits_equal_host_statement"] = bool(torch.equal(canvas[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(canvas[1], got[1])
                                                   and torch.equal(out[0][n:].view(torch.int32), got[2].view(torch.int32))
                                                   and torch.equal(out[1][n:], got[3]))
    rec["host_over_gather_eager"] = rec["host_gather_plus_upload_wall_ms"] / rec["gather_eager_ms"]
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    assemble()
    clean, label = out[0].clone(), out[1].clone()
    noisy = basic_operations.add_input_noise(clean, seed=1)
    _, t, lo, hi = timed(lambda: solver.cooperative_step(clean, label, noisy, IMG_CFG, SEG_CFG), args.device_reps, 5)
    rec["cooperative_step_ms"], rec["cooperative_step_ms_min_max"] = t * 1e3, [lo * 1e3, hi * 1e3]
    rec["assemble_over_cooperative_step"] = rec["assemble_eager_ms"] / rec["cooperative_step_ms"]
    rec["next_batch_over_cooperative_step"] = rec["next_batch_wall_ms"] / rec["cooperative_step_ms"]
    print(json.dumps(rec), flush=True)
    res = {"what": "one training batch of a device-resident set: gather = ops.batch_gather (canvas batch + original pair, one launch), assemble "
                   "= gather + BatchAugmenter.apply into the first half; device time between HIP events (median, warm), eager and as the "
                   "replay of one captured graph; next_batch = DeviceBatchLoader.next_batch wall time (order, draw, pinned copies, "
                   "launches, synchronised); host_gather_plus_upload = loader.gather_host (numpy) for the same indices plus the pinned "
                   "upload of its four arrays, wall time on the same machine; cooperative_step = one eager fp32 step on a batch of the "
                   "same size",
           "thresholds": "none: nothing was known about these times before this file was written",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "rocm": torch.version.hip,
           "torch": torch.__version__, "numpy": np.__version__, "host_cpus_usable": len(os.sched_getaffinity(0)), "result": rec}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
