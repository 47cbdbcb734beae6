"""Plan identity gate of the plan compiler (nets.py): compiles every plan the engine can ask for on device="cpu" and prints one line per
plan -- a SHA-256 over its op records (`ops`, `main_ops`, `tail_ops`, `table_np`), a SHA-256 over its record (`Plan.rec`, named tuples
flattened to plain tuples) and (n_ops, act_bytes, scr_bytes, bscr_bytes, out_shapes, groups, pro_entries, len(bn_log)).  Nothing is launched.

A refactor of the compiler leaves the output of this script unchanged: run it on both trees (`python tools/plan_digest.py > a.txt`) and
`cmp` the files.  The digests are NOT a golden file: every tuning of the tile heuristics changes them, and on a machine without a GPU the
occupancy queries of the library answer with a constant, so grids, statistics row counts and scratch sizes are the real ones only on one.

Matrix: (dtype, reduce_factor) in (fp32, 4), (bf16, 4), (fp32, 8) x Dropout2d off / 0.25 / 0.25 with an injected keep pattern x the five
networks (+ each network's pack plan) x five input sizes (three small ones, the two batches of bench.py's step) x BatchNorm mode A / B / C x 1 or 2 BatchNorm groups; per forward plan every
backward plan (output-gradient masks, need_dx x need_w); the pass-stack slots (0, 2), (1, 2) and the stacked backward over them
(gamma / beta mask x split tail); the code_decoupler-only plan."""
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cooperative_training_and_latent_space_data_augmentation_amd import nets        # noqa: E402

CONFIGS = [("fp32", 4), ("bf16", 4), ("fp32", 8)]
ENC_SIZES = [(2, 48, 64), (3, 80, 112), (4, 40, 56), (16, 256, 256), (32, 256, 256)]      # (the last two: the batches of bench.py's step)
DEC_SIZES = [(2, 3, 4), (3, 5, 7), (4, 4, 4), (16, 16, 16), (32, 16, 16)]                  # (the odd sizes reach the zero-insert data gradient)
DROPOUT = [("nodrop", None, False), ("drop", 0.25, False), ("dropkeep", 0.25, True)]


def compile_forward(net, n, h, w, mode, groups=1, pp=(0, 1)):
    return net._compile_forward(n, h, w, mode, groups=groups, pp=pp)


def compile_backward(net, fwd, mode, mask, need_dx, need_w, affine, affine_mask=0, split_tail=False):
    return net._compile_backward(fwd, mode, mask, need_dx, need_w, affine, affine_mask=affine_mask, split_tail=split_tail)


def plain(obj):
    """a plan record with every (named) tuple as a plain tuple: what a reader that indexes positionally sees"""
    if isinstance(obj, dict):
        return {k: plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return tuple(plain(v) for v in obj)
    return obj


def line(label, p):
    h = hashlib.sha256()
    for a in (p.ops, p.main_ops, p.tail_ops, p.table_np):
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes() + b"|")
    rec = hashlib.sha256(repr(plain(p.rec)).encode()).hexdigest()[:16]
    out_shapes = None if p.out_shapes is None else [tuple(s) for s in p.out_shapes]
    print(label, h.hexdigest(), rec, (p.n_ops, p.act_bytes, p.scr_bytes, p.bscr_bytes, out_shapes, p.groups, p.pro_entries, len(p.bn_log)))
    return 1


def backward_cases(name):
    masks = [(True, True), (True, False), (False, True)] if name == "image_encoder" else [(True,)]
    return list(itertools.product(masks, (False, True), (False, True)))


def main():
    rows = 0
    for dtype, rf in CONFIGS:
        model = nets.build_networks(reduce_factor=rf, device="cpu", dtype=dtype)
        for name, net in model.items():
            rows += line(f"{dtype}/{rf} {name} pack", net._pack_plan)
        for tag, p_drop, keep in DROPOUT:
            for name, net in model.items():
                net.set_dropout(p_drop)
                net.set_dropout_keep([torch.ones(1, 1)] if keep else None)      # (a compile only asks whether patterns are injected)
                for n, h, w in (ENC_SIZES if name.endswith("encoder") else DEC_SIZES):
                    head = f"{dtype}/{rf} {tag} {name} {n}x{h}x{w}"
                    for mode, groups in itertools.product("ABC", (1, 2) if n % 2 == 0 else (1,)):
                        fwd = compile_forward(net, n, h, w, mode, groups)
                        rows += line(f"{head} {mode} g{groups} fwd", fwd)
                        for mask, need_dx, need_w in backward_cases(name):
                            b = compile_backward(net, fwd, mode, mask, need_dx, need_w, mode == "A")
                            rows += line(f"{head} {mode} g{groups} bwd {mask} dx{int(need_dx)} w{int(need_w)}", b)
                        if mode == "C":
                            continue
                        # the pass stack: two slots of one arena, one backward over the stacked view of slot 0
                        p0 = compile_forward(net, n, h, w, mode, groups, (0, 2))
                        rows += line(f"{head} {mode} g{groups} slot0", p0)
                        rows += line(f"{head} {mode} g{groups} slot1", compile_forward(net, n, h, w, mode, groups, (1, 2)))
                        view = nets._StackedForward(nets._stack_rec(p0.rec, 2), 2 * groups)
                        full = backward_cases(name)[0][0]
                        for amask, split, need_dx in itertools.product((0, (1 << groups) - 1), (False, True), (False, True)):
                            b = compile_backward(net, view, "A", full, need_dx, True, True, amask, split)
                            rows += line(f"{head} {mode} g{groups} stacked a{amask} s{int(split)} dx{int(need_dx)}", b)
                    if name == "image_encoder":
                        for mode in "ABC":
                            rows += line(f"{head} {mode} filter", net._compile_filter(n, h // 16, w // 16, mode))
    print(f"# {rows} plans", file=sys.stderr)


if __name__ == "__main__":
    main()
