"""Test-time augmentation kernels (csrc/ctl_tta.hip) at volume sizes: an image volume n x 1 x H x W and the network's logits on its
views, T*n x 4 x H x W, for 10 x 192 x 192 and 40 x 256 x 256.

Per size and view set ("flips", "d4", and the transposing codes (1, 3, 5, 7) beside "flips", which has the same T without a transpose):
  views, merge, views_merge   device time between HIP events, warm, median over repeated batches of `--inner` calls divided by the batch:
                              the calls as issued from Python (eager) and the replay of one captured graph.  merge in "prob" mode writes
                              merged + pred, with and without `aligned`; "logit" mode is recorded for merged + pred.
  aten                        the same results from the ATen composition (flip / transpose / contiguous per view; the inverse per member,
                              softmax, mean, argmax), eager
  predict                     solver.predict over the T*n stack (random weights, FCN_16_standard): what the two launches sit around
  bytes                       what the algorithm must move: views read n*H*W*4 and write T*n*H*W*4; merge reads T*n*C*H*W*4 and writes the
                              outputs asked for; bytes / graph time against the achievable HBM rate of 6.3 TB/s (8 TB/s peak)
The device results are compared with the ATen composition at the smaller size (views and aligned: equal bits; merged: max abs difference).
Nothing is asserted about the times.  CTL_TOOL_LIB=<variant> (tools/_variant.py) measures another build of the library, e.g. one compiled
with -DCTL_TTA_STRIDED=1 (transposed views read one pixel per source row instead of going through the LDS tile); its name is recorded.
Writes profiles/tta.json.

    python tools/bench_tta.py [--out profiles/tta.json] [--reps 20] [--inner 10] [--sizes small,large]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _variant  # noqa: E402

_variant.use_variant()

from bench_cc import device_ms  # noqa: E402
from bench_restore import captured  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops, tta  # noqa: E402

SIZES = {"small": (10, 4, 192, 192), "large": (40, 4, 256, 256)}
SETS = {"flips": "flips", "d4": "d4", "transposing": (1, 3, 5, 7)}
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12


def view_aten(x, v):
    a = x.transpose(-1, -2) if v & 1 else x
    a = torch.flip(a, dims=(-2,)) if v & 2 else a
    return torch.flip(a, dims=(-1,)) if v & 4 else a


def unview_aten(y, v):
    a = torch.flip(y, dims=(-1,)) if v & 4 else y
    a = torch.flip(a, dims=(-2,)) if v & 2 else a
    return a.transpose(-1, -2) if v & 1 else a


def aten_views(image, codes):
    return torch.cat([view_aten(image, v).contiguous(memory_format=torch.channels_last) for v in codes], 0)


def aten_merge(logits, codes, mode, want_aligned):
    n = logits.shape[0] // len(codes)
    members = [unview_aten(logits[t * n:(t + 1) * n], v).contiguous(memory_format=torch.channels_last) for t, v in enumerate(codes)]
    stack = torch.stack(members, 0)
    merged = (torch.softmax(stack, 2) if mode == "prob" else stack).mean(0)
    return (stack.flatten(0, 1) if want_aligned else None), merged, merged.argmax(1).to(torch.uint8)


def per_call(fn, reps, inner):
    med, lo, hi = device_ms(lambda: [fn() for _ in range(inner)], reps)
    return {"ms": med / inner, "ms_min_max": [lo / inner, hi / inner]}


def both(fn, reps, inner):
    rec = {"eager": per_call(fn, reps, inner)}
    graph = captured(fn)
    rec["graph"] = per_call(graph.replay, reps, inner)
    del graph
    return rec


def with_bytes(rec, nbytes):
    rate = nbytes / (rec["graph"]["ms"] * 1e-3)
    rec.update(bytes=nbytes, bytes_per_s_graph=rate, share_of_achievable_hbm=rate / HBM_ACHIEVABLE, share_of_peak_hbm=rate / HBM_PEAK)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", default="small,large")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py measures on the GPU: no device found")
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    rows = {}
    for size in args.sizes.split(","):
        n, c, h, w = SIZES[size]
        g = torch.Generator().manual_seed(n)
        image = torch.rand(n, 1, h, w, generator=g).cuda()
        for name, spec in SETS.items():
            codes = tta.parse_views(spec)
            T = len(codes)
            logits = (torch.randn(T * n, h, w, c, generator=g) * 3.0).permute(0, 3, 1, 2).cuda()
            px = n * h * w
            rec = {"T": T, "codes": list(codes)}
            rec["views"] = with_bytes(both(lambda: ops.tta_views(image, codes), args.reps, args.inner), px * 4 + T * px * 4)
            for mode, aligned in (("prob", False), ("prob", True), ("logit", False)):
                want = (("aligned",) if aligned else ()) + ("merged", "pred")
                key = f"merge_{mode}" + ("_aligned" if aligned else "")
                nbytes = T * px * c * 4 + px * c * 4 + px + (T * px * c * 4 if aligned else 0)
                rec[key] = with_bytes(both(lambda: ops.tta_merge(logits, codes, (h, w), mode=mode, want=want), args.reps, args.inner), nbytes)
                rec[key]["aten_eager"] = per_call(lambda: aten_merge(logits, codes, mode, aligned), args.reps, max(args.inner // 4, 2))
                rec[key]["aten_eager_over_graph"] = rec[key]["aten_eager"]["ms"] / rec[key]["graph"]["ms"]
                rec[key]["aten_eager_over_eager"] = rec[key]["aten_eager"]["ms"] / rec[key]["eager"]["ms"]
            rec["views"]["aten_eager"] = per_call(lambda: aten_views(image, codes), args.reps, max(args.inner // 4, 2))
            rec["views"]["aten_eager_over_graph"] = rec["views"]["aten_eager"]["ms"] / rec["views"]["graph"]["ms"]

            def chain():
                ops.tta_views(image, codes)
                return ops.tta_merge(logits, codes, (h, w), mode="prob", want=("aligned", "merged", "pred"))

            def aten_chain():
                aten_views(image, codes)
                return aten_merge(logits, codes, "prob", True)

            rec["views_merge_prob_aligned"] = both(chain, args.reps, args.inner)
            rec["views_merge_prob_aligned"]["aten_eager"] = per_call(aten_chain, args.reps, max(args.inner // 4, 2))
            rec["views_merge_prob_aligned"]["aten_eager_over_graph"] = (rec["views_merge_prob_aligned"]["aten_eager"]["ms"] /
                                                                       rec["views_merge_prob_aligned"]["graph"]["ms"])
            stack = ops.tta_views(image, codes)
            rec["predict_stack"] = per_call(lambda: solver.predict(input=stack, softmax=False), max(args.reps // 4, 3), 1)
            rec["views_merge_graph_over_predict"] = rec["views_merge_prob_aligned"]["graph"]["ms"] / rec["predict_stack"]["ms"]
            if size == "small":
                got = ops.tta_merge(logits, codes, (h, w), mode="prob", want=("aligned", "merged", "pred"))
                ref = aten_merge(logits, codes, "prob", True)
                rec["check"] = {"views_equal_bits": bool(torch.equal(stack, aten_views(image, codes))),
                                "aligned_equal_bits": bool(torch.equal(got.aligned, ref[0])),
                                "merged_max_abs_diff_to_aten": float((got.merged - ref[1]).abs().max()),
                                "pred_mismatches_to_aten": int((got.pred != ref[2]).sum())}
            rows[f"{n}x{c}x{h}x{w} {name}"] = rec
            print(json.dumps({f"{n}x{c}x{h}x{w} {name}": rec}), flush=True)
            del logits, stack
            torch.cuda.empty_cache()
    res = {"what": "ops.tta_views (image n x 1 x H x W) and ops.tta_merge (logits T*n x 4 x H x W, fp32 NHWC): device time between HIP events per "
                   f"call (median of {args.reps} batches of {args.inner} calls, warm), eager and as the replay of one captured graph; aten_eager = "
                   "the same results from flip / transpose / contiguous / softmax / mean / argmax; predict_stack = solver.predict over the T*n "
                   "stack (random weights, FCN_16_standard); bytes = what the algorithm must read and write",
           "library": os.path.relpath(_ffi.LIB_PATH, ROOT), "thresholds": "none", "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "rocm": torch.version.hip, "torch": torch.__version__, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
