"""The argument contract of the ops wrappers that take caller-supplied outputs or typed tensor inputs: which exception class a
malformed tensor raises, and that a well-formed `out` comes back as the same object.  One row per (wrapper, argument, defect); the
classes are the ones the wrappers raised before their checks were gathered into shared helpers, so the table pins them.

Shapes are the smallest that reach the checks and still run: 16x16 planes with an 8x8 crop for the warps (n = 2), 128x128 for the
bias field (the smallest side it accepts), 2x4x4 volumes, two 4x4 slices for the arena entries, a 4x4 window on a 6x6 native grid."""
import collections

import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops, prepare

pytestmark = pytest.mark.gpu

F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8
OTHER = {F32: torch.float64, I64: I32, I32: I64, U8: I32}

# make() -> fresh well-formed tensors by argument name; run(args) -> the wrapper's result; outs: output name -> index into the result
# (None: the result is the output); inputs: typed input name -> a wrong shape for it
Case = collections.namedtuple("Case", "make run outs inputs")


def rand(*shape):
    return torch.rand(shape, dtype=F32, device="cuda")


def empty(dtype, *shape):
    return torch.empty(shape, dtype=dtype, device="cuda")


def identity_map(n):
    return torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], device="cuda").repeat(n, 1, 1)


def unit_intensity(n):
    return torch.tensor([[1.0, 0.0]], device="cuda").repeat(n, 1)


def arenas():
    label = (torch.arange(32, device="cuda") % 3).to(U8)
    return {"image_arena": rand(32), "label_arena": label, "table": torch.tensor([[0, 4, 4], [16, 4, 4]], dtype=I64, device="cuda")}


GEOMETRY = prepare.geometry(2, 6, 6, crop_size=(4, 4))
SPIKE_K, SPIKE_MULT = np.int32([[0, 1, 1]]), np.int32([2])

CASES = {
    "aug_elastic_field": Case(
        lambda: {"noise": rand(2, 2, 16, 16), "out": empty(F32, 2, 2, 16, 16)},
        lambda a: ops.aug_elastic_field(2, 16, 16, 3.0, 2.0, 5, noise=a["noise"], out=a["out"]),
        {"out": None}, {"noise": (2, 2, 16, 15)}),
    "aug_bias_field": Case(
        lambda: {"image": rand(1, 1, 128, 128), "bias": torch.zeros((1, ops.BIAS_FLOATS), device="cuda"), "noise": rand(1, 1, 128, 128),
                 "out": empty(F32, 1, 1, 128, 128)},
        lambda a: ops.aug_bias_field(a["image"], a["bias"], seed=1, noise=a["noise"], out=a["out"]),
        {"out": None}, {"image": (1, 2, 128, 128), "bias": (1, ops.BIAS_FLOATS - 1), "noise": (1, 1, 128, 127)}),
    "aug_coarse_field": Case(
        lambda: {"coarse": torch.zeros((2, ops.COARSE_FLOATS), device="cuda"), "out": empty(F32, 2, 2, 16, 16)},
        lambda a: ops.aug_coarse_field(2, 16, 16, a["coarse"], out=a["out"]),
        {"out": None}, {"coarse": (2, ops.COARSE_FLOATS - 6)}),
    "aug_spline_coeffs": Case(
        lambda: {"image": rand(2, 1, 16, 16), "intensity": unit_intensity(2), "out": empty(F32, 2, 1, 16, 16)},
        lambda a: ops.aug_spline_coeffs(a["image"], intensity=a["intensity"], out=a["out"]),
        {"out": None}, {"image": (2, 2, 16, 16), "intensity": (2, 3)}),
    "aug_warp": Case(
        lambda: {"image": rand(2, 1, 16, 16), "label": torch.zeros((2, 16, 16), dtype=I64, device="cuda"), "matrix": identity_map(2),
                 "intensity": unit_intensity(2), "field": torch.zeros((2, 2, 16, 16), device="cuda"),
                 "out[0]": empty(F32, 2, 1, 8, 8), "out[1]": empty(I64, 2, 8, 8)},
        lambda a: ops.aug_warp(a["image"], a["label"], a["matrix"], a["intensity"], (8, 8), field=a["field"], out=(a["out[0]"], a["out[1]"])),
        {"out[0]": 0, "out[1]": 1},
        {"image": (2, 2, 16, 16), "label": (2, 16, 15), "matrix": (2, 2, 4), "intensity": (2, 3), "field": (2, 2, 16, 15)}),
    "rescale_intensity": Case(
        lambda: {"data": rand(2, 1, 4, 4), "out": empty(F32, 2, 1, 4, 4)},
        lambda a: ops.rescale_intensity(a["data"], out=a["out"]), {"out": None}, {}),
    "percentile_normalize": Case(
        lambda: {"x": rand(2, 4, 4), "out": empty(F32, 2, 4, 4)},
        lambda a: ops.percentile_normalize(a["x"], out=a["out"]), {"out": None}, {}),
    "keep_largest_components": Case(
        lambda: {"labelmap": (torch.arange(32, device="cuda") % 4).to(U8).reshape(2, 4, 4), "out": empty(U8, 2, 4, 4)},
        lambda a: ops.keep_largest_components(a["labelmap"], 4, out=a["out"]), {"out": None}, {}),
    "restore_scores": Case(
        lambda: {"scores": rand(2, 3, 4, 4), "out": empty(U8, 2, 6, 6)},
        lambda a: ops.restore_scores(a["scores"], GEOMETRY, out=a["out"]), {"out": None}, {}),
    "restore_labels": Case(
        lambda: {"labels": (torch.arange(32, device="cuda") % 3).to(U8).reshape(2, 4, 4), "out": empty(U8, 2, 6, 6)},
        lambda a: ops.restore_labels(a["labels"], GEOMETRY, out=a["out"]), {"out": None}, {}),
    "corrupt_bias_field": Case(
        lambda: {"x": rand(2, 4, 4), "out": empty(F32, 2, 4, 4)},
        lambda a: ops.corrupt_bias_field(a["x"], np.zeros(20), out=a["out"]), {"out": None}, {}),
    "corrupt_spike": Case(
        lambda: {"x": rand(2, 4, 4), "out": empty(F32, 2, 4, 4)},
        lambda a: ops.corrupt_spike(a["x"], SPIKE_K, SPIKE_MULT, 0.5, out=a["out"]), {"out": None}, {}),
    "corrupt_rigid3d": Case(
        lambda: {"x": rand(2, 4, 4), "out": empty(F32, 1, 2, 4, 4)},
        lambda a: ops.corrupt_rigid3d(a["x"], np.eye(3, 4)[None], out=a["out"]), {"out": None}, {}),
    "axis_operator": Case(
        lambda: {"x": rand(2, 4, 4), "stack": rand(1, 2, 4, 4), "matrix": rand(4, 8), "out": empty(F32, 2, 4, 4)},
        lambda a: ops.axis_operator(a["x"], a["matrix"], 2, stack=a["stack"], out=a["out"]),
        {"out": None}, {"stack": (1, 2, 4, 5), "matrix": (4, 9)}),
    "resample_inplane": Case(
        lambda: {"image": rand(2, 4, 4), "label": (torch.arange(32, device="cuda") % 3).to(U8).reshape(2, 4, 4)},
        lambda a: ops.resample_inplane(a["image"], (1.0, 1.0, 5.0), (2.0, 2.0, -1.0), label=a["label"]),
        {}, {"image": (2, 1, 4, 4), "label": (2, 4, 5)}),
    "slice_foreground": Case(
        lambda: dict(arenas(), out=empty(I32, 2)),
        lambda a: ops.slice_foreground(a["label_arena"], a["table"], out=a["out"]), {"out": None}, {}),
    "batch_gather": Case(
        lambda: dict(arenas(), **{"out[0]": empty(F32, 2, 1, 4, 4), "out[1]": empty(I64, 2, 4, 4),
                                  "orig_out[0]": empty(F32, 2, 1, 4, 4), "orig_out[1]": empty(I64, 2, 4, 4)}),
        lambda a: ops.batch_gather(a["image_arena"], a["label_arena"], a["table"], torch.tensor([1, 0], dtype=I32, device="cuda"),
                                   torch.arange(256, device="cuda").to(U8), (4, 4), crop=(4, 4), out=(a["out[0]"], a["out[1]"]),
                                   orig_out=(a["orig_out[0]"], a["orig_out[1]"])),
        {"out[0]": 0, "out[1]": 1, "orig_out[0]": 2, "orig_out[1]": 3}, {}),
}

# a host `out` reaches require_gpu (CtlError) before or instead of the output check at these wrappers; everywhere else it is a ValueError
HOST_OUT_IS_CTL_ERROR = {"restore_scores", "restore_labels", "slice_foreground", "batch_gather"}
# `out` must not be this input
NOT_THE_INPUT = {"rescale_intensity": "data", "percentile_normalize": "x"}


def widened(t, by):
    return tuple(t.shape[:-1]) + (by(t.shape[-1]),)


DEFECTS = {
    "dtype": lambda t, bad_shape: t.to(OTHER[t.dtype]),
    "shape": lambda t, bad_shape: torch.zeros(bad_shape or widened(t, lambda v: v + 1), dtype=t.dtype, device=t.device),
    "strided": lambda t, bad_shape: torch.zeros(widened(t, lambda v: 2 * v), dtype=t.dtype, device=t.device)[..., ::2],
    "host": lambda t, bad_shape: t.cpu(),
}


def rows():
    for who, case in CASES.items():
        for name in case.outs:
            for defect in ("dtype", "shape", "strided", "host"):
                ctl = defect == "host" and who in HOST_OUT_IS_CTL_ERROR
                yield who, name, defect, _ffi.CtlError if ctl else ValueError
        if who in NOT_THE_INPUT:
            yield who, "out", "input", ValueError
        for name in case.inputs:
            for defect in ("dtype", "shape"):
                yield who, name, defect, ValueError


ROWS = list(rows())


@pytest.mark.parametrize("who,name,defect,error", ROWS, ids=[f"{w}-{n}-{d}" for w, n, d, _ in ROWS])
def test_malformed_argument_raises_its_class(who, name, defect, error):
    case = CASES[who]
    args = case.make()
    result = case.run(args)                                          # the well-formed call: every supplied output is handed back
    for out_name, index in case.outs.items():
        got = result if index is None else result[index]
        assert got is args[out_name] and got.data_ptr() == args[out_name].data_ptr(), (who, out_name)
    bad = case.make()
    bad[name] = bad[NOT_THE_INPUT[who]] if defect == "input" else DEFECTS[defect](bad[name], case.inputs.get(name))
    if defect == "strided":
        assert not bad[name].is_contiguous() and bad[name].shape == args[name].shape
    with pytest.raises(error) as info:
        case.run(bad)
    assert type(info.value) is error, (who, name, defect, type(info.value))       # CtlError is a RuntimeError, never a ValueError
    if error is ValueError:                                          # the message names the wrapper and the argument
        assert who in str(info.value) and name.split("[")[0] in str(info.value), str(info.value)
