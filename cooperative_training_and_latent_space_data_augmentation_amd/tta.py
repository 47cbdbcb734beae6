"""Test-time augmentation over the dihedral group of the square (a project addition, off by default; upstream has no counterpart).

Predict several flipped / rotated views of a volume, undo the transform on the logits and average.  `predict` runs in eval mode, so T
views of n slices are ONE pass over T * n slices; around it sit two launches, `ops.tta_views` and `ops.tta_merge` (csrc/ctl_tta.hip).

A view is coded v = 0..7: bit 0 = transpose, bit 1 = flip along H, bit 2 = flip along W, applied in that order.  This module holds
  VIEW_SETS, parse_views      the named sets and the one place a view specification is checked
  views_host, merge_host      the numpy statements the kernels are tested against, written with np.flip / np.swapaxes (the kernels use
                              an index formula), called by nothing on the device path
  predict_tta                 views -> one `predict` over the stack -> merge
"""
from collections import namedtuple

import numpy as np

VIEW_SETS = {"flips": (0, 2, 4, 6), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
MODES = ("logit", "prob")

HostTtaMerge = namedtuple("HostTtaMerge", "aligned merged pred")


def parse_views(spec, hw=None):
    """A view set as a tuple of distinct codes: "flips", "d4", or 1 to 8 distinct integers 0..7 (the identity need not be among them).
    hw: the plane (H, W) the views are for; a transposing code needs H == W.  ValueError otherwise, naming the code."""
    codes = _parse(spec)
    if hw is not None and int(hw[0]) != int(hw[1]):
        for v in codes:
            if v & 1:
                raise ValueError(f"tta: view code {v} transposes, the plane {int(hw[0])} x {int(hw[1])} is not square")
    return codes


def _parse(spec):
    if isinstance(spec, str):
        if spec not in VIEW_SETS:
            raise ValueError(f"tta: unknown view set {spec!r} (one of {', '.join(sorted(VIEW_SETS))}, or a tuple of codes 0..7)")
        return VIEW_SETS[spec]
    try:
        codes = tuple(spec)
    except TypeError:
        raise ValueError(f"tta: views {spec!r}: a set name or a tuple of codes 0..7") from None
    if not 1 <= len(codes) <= 8:
        raise ValueError(f"tta: {len(codes)} views (1 .. 8)")
    for v in codes:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 7:
            raise ValueError(f"tta: view code {v!r} (an integer 0 .. 7)")
    codes = tuple(int(v) for v in codes)
    for v in codes:
        if codes.count(v) > 1:
            raise ValueError(f"tta: duplicate view code {v}")
    return codes


def _view(x, v):
    """view v of the planes on the last two axes of x"""
    a = np.swapaxes(x, -1, -2) if v & 1 else x
    a = np.flip(a, axis=-2) if v & 2 else a
    return np.flip(a, axis=-1) if v & 4 else a


def _unview(y, v):
    """the planes whose view v is y: the flips undone, then the transpose"""
    a = np.flip(y, axis=-1) if v & 4 else y
    a = np.flip(a, axis=-2) if v & 2 else a
    return np.swapaxes(a, -1, -2) if v & 1 else a


def views_host(x, views):
    """[n, c, H, W] -> [T * n, c, H, W], member-major: member t is view views[t] of every slice (dtype kept)."""
    x = np.asarray(x)
    if x.ndim != 4:
        raise ValueError(f"views_host: expected [n, c, H, W], got {x.shape}")
    codes = parse_views(views, x.shape[-2:])
    return np.ascontiguousarray(np.concatenate([_view(x, v) for v in codes], axis=0))


def merge_host(logits, views, hw, mode="prob"):
    """logits [T * n, C, H, W] on the views (member-major), hw = the native (H, W) -> HostTtaMerge:
      aligned  [T * n, C, H, W], every member back on the native grid (dtype kept: a permutation);
      merged   [n, C, H, W]: mode "prob" -> float64, the mean over the members of the softmax of the float64 logits (mean_prob of
               uncertainty.predictive_stats_host); mode "logit" -> float32, literally (((x_0 + x_1) + ..) + x_T-1) / float32(T);
      pred     [n, H, W] uint8, the first maximum of merged.
    mode=None: aligned alone."""
    x = np.asarray(logits)
    h, w = (int(v) for v in hw)
    codes = parse_views(views, (h, w))
    T = len(codes)
    if x.ndim != 4 or x.shape[0] % T or tuple(x.shape[2:]) != (h, w):
        raise ValueError(f"merge_host: expected [{T} * n, C, {h}, {w}] logits, got {x.shape}")
    if mode is not None and mode not in MODES:
        raise ValueError(f"merge_host: mode {mode!r}, one of {MODES} or None")
    n = x.shape[0] // T
    members = [np.ascontiguousarray(_unview(x[t * n:(t + 1) * n], v)) for t, v in enumerate(codes)]
    aligned = np.concatenate(members, axis=0)
    if mode is None:
        return HostTtaMerge(aligned, None, None)
    if mode == "prob":
        z = aligned.astype(np.float64).reshape(T, n, *aligned.shape[1:])
        z = z - z.max(axis=2, keepdims=True)
        p = np.exp(z) / np.exp(z).sum(axis=2, keepdims=True)
        merged = p.sum(axis=0) / float(T)
    else:
        acc = members[0].astype(np.float32)
        for m in members[1:]:
            acc = acc + m.astype(np.float32)
        merged = acc / np.float32(T)
    return HostTtaMerge(aligned, merged, merged.argmax(axis=1).astype(np.uint8))


def predict_tta(solver, image, views, mode="prob", n_iter=None, want=("merged",)):
    """Test-time augmentation of one device batch `image` [n, 1..4, H, W]: ops.tta_views, ONE solver.predict(softmax=False) over the
    T * n stack (eval mode: slices are independent, batching is bitwise neutral), ops.tta_merge -> ops.TtaMerge(aligned, merged, pred)
    with what `want` names.  mode "prob" (the default: the calibration columns are defined on the mean probability) averages the
    members' softmax, "logit" their logits."""
    from . import ops
    codes = parse_views(views, image.shape[-2:])
    stack = ops.tta_views(image, codes)
    logits = solver.predict(input=stack, softmax=False, n_iter=n_iter)
    return ops.tta_merge(logits, codes, image.shape[-2:], mode=mode, want=want)
