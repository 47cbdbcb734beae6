"""Predictive uncertainty and calibration (medseg/common_utils/uncertainty.py:7-54; the Brier sum of medseg/models/custom_loss.py:495-511).

Device path: `ops.predictive_stats` (csrc/ctl_uncert.hip), one streaming pass over logits that are already on the device.  This module
holds what sits around it:
  cal_entropy_maps / cal_batch_entropy_maps   upstream's two functions, names and arguments kept: numpy in -> upstream's arithmetic
                                              restated in numpy; CUDA tensor in -> the kernel with is_prob=True
  predictive_stats_host                       the float64 host statement of include/ctl_hip.h "predictive uncertainty": the definition the
                                              kernel is tested against, called by nothing on the device path
  calibration_from_tables                     ECE / NLL / Brier / Entropy / accuracy from the two small tables, in float64
  cooperative_members                         the FTN / STN two-member ensemble of a cooperative model, ready for members=2
  tta_members                                 the T-member ensemble over D4 views of the input (tta.py), ready for members=T
"""
from collections import namedtuple

import numpy as np

CALIBRATION_METRICS = ("ECE", "NLL", "Brier", "Entropy")
CONF_SCALE = 2 ** 32      # the device adds conf * 2^32 as an integer (include/ctl_hip.h)

# the fields of ops.PredictiveStats, then the per-pixel nll / brier maps behind the two sums (NaN at unlabelled pixels)
HostPredictiveStats = namedtuple("HostPredictiveStats", "entropy mi conf pred mean_prob stats bins nll brier")


# ---------------------------------------------------------------------------------------------- upstream's entropy maps
def _entropy_numpy(pred_probs, eps, threhold, use_max, axis):
    if use_max:
        ax_probs = np.amax(pred_probs, axis=axis)
        entropy = (-ax_probs * np.log2(ax_probs + eps))
    else:
        entropy = (-pred_probs * np.log2(pred_probs + eps)).sum(axis=axis)
    entropy = np.nan_to_num(entropy)
    entropy[entropy < threhold] = 0.
    return entropy


def _entropy_device(probs, eps, threhold, use_max):
    """probs: CUDA tensor [N,C,H,W] of probabilities -> fp32 device tensor [N,H,W]"""
    import torch
    from . import ops
    if use_max:      # upstream's form: -max_k p_k * log2(max_k p_k + eps), from the kernel's confidence map
        conf = ops.predictive_stats(probs, eps=eps, is_prob=True, want=("conf",)).conf
        entropy = -conf * torch.log2(conf + eps)
    else:
        entropy = ops.predictive_stats(probs, eps=eps, is_prob=True, want=("entropy",)).entropy
    entropy = torch.nan_to_num(entropy)
    entropy[entropy < threhold] = 0.
    return entropy


def _is_device_tensor(x) -> bool:
    import torch
    return torch.is_tensor(x) and x.is_cuda


def cal_entropy_maps(pred_probs, eps=1e-7, threhold=0., use_max=False):
    """uncertainty.py:7-27: entropy map [H,W] in bits of ONE image's softmax output [C,H,W]; values under `threhold` become 0.  use_max:
    -p log2(p + eps) of the largest probability alone instead of the sum over the classes.  A CUDA tensor gives a CUDA tensor."""
    assert len(pred_probs.shape) == 3, 'only support input of three dimension [Channel, H, W]'
    if _is_device_tensor(pred_probs):
        return _entropy_device(pred_probs[None], eps, threhold, use_max)[0]
    return _entropy_numpy(np.asarray(pred_probs), eps, threhold, use_max, 0)


def cal_batch_entropy_maps(pred_probs, eps=1e-7, threhold=0., use_max=False):
    """uncertainty.py:30-54: the same for a batch [N,C,H,W] -> [N,H,W]."""
    assert len(pred_probs.shape) == 4, 'only support input of four dimension [N, Channel, H, W]'
    if _is_device_tensor(pred_probs):
        return _entropy_device(pred_probs, eps, threhold, use_max)
    return _entropy_numpy(np.asarray(pred_probs), eps, threhold, use_max, 1)


# ---------------------------------------------------------------------------------------------- the host statement
def bin_edges(n_bins: int) -> np.ndarray:
    """The inner edges float32(j) / float32(n_bins), j = 1..n_bins-1, as the kernel rounds them, widened to float64."""
    return (np.arange(1, n_bins, dtype=np.float32) / np.float32(n_bins)).astype(np.float64)


def _entropy_bits(p, eps, axis):
    q = p + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(q > 0, p * np.log2(np.where(q > 0, q, 1.0)), 0.0)
    return -term.sum(axis=axis)


def predictive_stats_host(logits, label=None, members=1, n_bins=15, eps=1e-7, is_prob=False):
    """The definition of include/ctl_hip.h "predictive uncertainty" in float64.  logits: [T*n, C, H, W], member-major (any float type, read
    as float64); label: [n, H, W] integers or None; a label outside 0..C-1 is unlabelled.  -> HostPredictiveStats: entropy / mi / conf
    [n,H,W] float64 (bits), pred [n,H,W] uint8, mean_prob [n,C,H,W], stats [n,6] (labelled, correct, sum H, sum MI, sum nll, sum brier),
    bins [n,n_bins,3] float64 (count, correct, sum conf), and the per-pixel nll / brier maps (NaN where unlabelled)."""
    x = np.asarray(logits, dtype=np.float64)
    T, B = int(members), int(n_bins)
    if x.ndim != 4 or T < 1 or x.shape[0] % T:
        raise ValueError(f"predictive_stats_host: expected [members * n, C, H, W] logits, got {x.shape} for {T} members")
    if not 1 <= B <= 64 or not 1 <= x.shape[1] <= 16 or not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"predictive_stats_host: n_bins {B} (1..64), classes {x.shape[1]} (1..16), eps {eps} (finite, >= 0)")
    n, (c, h, w) = x.shape[0] // T, x.shape[1:]
    x = x.reshape(T, n, c, h, w)
    with np.errstate(divide="ignore"):
        if is_prob:
            p, logp = x, np.log(x)
        else:
            z = x - x.max(axis=2, keepdims=True)
            s = np.exp(z).sum(axis=2, keepdims=True)
            p, logp = np.exp(z) / s, z - np.log(s)
    pbar = p.sum(axis=0) / float(T)
    conf, pred = pbar.max(axis=1), pbar.argmax(axis=1)                    # argmax: the first maximum
    H = _entropy_bits(pbar, eps, 1)
    mi = H - _entropy_bits(p, eps, 2).sum(axis=0) / float(T) if T > 1 else np.zeros_like(H)
    stats, bins = np.zeros((n, 6)), np.zeros((n, B, 3))
    stats[:, 2], stats[:, 3] = H.sum(axis=(1, 2)), mi.sum(axis=(1, 2))
    nll, brier = np.full((n, h, w), np.nan), np.full((n, h, w), np.nan)
    if label is not None:
        y = np.asarray(label).astype(np.int64).reshape(n, h, w)
        valid = (y >= 0) & (y < c)
        yc = np.where(valid, y, 0)
        lp = np.take_along_axis(logp, np.broadcast_to(yc[None, :, None], (T, n, 1, h, w)), axis=2)[:, :, 0]      # [T,n,h,w]
        m = lp.max(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            lse = np.where(np.isfinite(m), m + np.log(np.exp(lp - np.where(np.isfinite(m), m, 0.0)).sum(axis=0)), m)
        onehot = (np.arange(c)[None, :, None, None] == yc[:, None])
        nll = np.where(valid, -(lse - np.log(float(T))), np.nan)
        brier = np.where(valid, ((pbar - onehot) ** 2).sum(axis=1), np.nan)
        correct = valid & (pred == y)
        which = (conf[..., None] > bin_edges(B)).sum(axis=-1)
        for b in range(n):
            v = valid[b]
            stats[b, 0], stats[b, 1] = v.sum(), correct[b].sum()
            stats[b, 4], stats[b, 5] = nll[b][v].sum(), brier[b][v].sum()
            bins[b, :, 0] = np.bincount(which[b][v], minlength=B)
            bins[b, :, 1] = np.bincount(which[b][correct[b]], minlength=B)
            bins[b, :, 2] = np.bincount(which[b][v], weights=conf[b][v], minlength=B)
    return HostPredictiveStats(H, mi, conf, pred.astype(np.uint8), pbar, stats, bins, nll, brier)


def calibration_from_tables(stats, bins, pixels=None):
    """{ECE, NLL, Brier, Entropy, accuracy} in float64 from the `stats` [n,6] and `bins` [n,B,3] tables of one or more slices (host arrays;
    the slices are pooled).  An integer `bins` table is the device's: its third column is the sum of conf * 2^32.  ECE = sum over the
    non-empty bins of (n_b / N) |correct_b / n_b - sum conf_b / n_b|; NLL and Brier are means over the N labelled pixels (NaN when there
    is none); Entropy is sum H / pixels in bits, `pixels` = the number of ALL pixels behind the tables (default: N, right when every
    pixel is labelled)."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 6).sum(axis=0)
    bins = np.asarray(bins)
    B = bins.shape[-2]
    fixed = np.issubdtype(bins.dtype, np.integer)
    flat = bins.reshape(-1, B, 3)
    count = [sum(int(v) for v in flat[:, j, 0]) for j in range(B)]
    right = [sum(int(v) for v in flat[:, j, 1]) for j in range(B)]
    if fixed:      # exact integer sums; one correctly rounded division each
        csum = [sum(int(v) for v in flat[:, j, 2]) / CONF_SCALE for j in range(B)]
    else:
        csum = [float(np.sum(flat[:, j, 2].astype(np.float64))) for j in range(B)]
    N = float(sum(count))
    nan = float("nan")
    if N == 0:
        ece = nll = brier = acc = nan
    else:
        ece = float(sum((count[j] / N) * abs(right[j] / count[j] - csum[j] / count[j]) for j in range(B) if count[j]))
        nll, brier, acc = float(stats[4] / N), float(stats[5] / N), float(sum(right) / N)
    total = N if pixels is None else float(pixels)
    return {"ECE": ece, "NLL": nll, "Brier": brier, "Entropy": float(stats[2] / total) if total else nan, "accuracy": acc}


# ---------------------------------------------------------------------------------------------- the FTN / STN ensemble
def cooperative_members(solver, image):
    """The two-member ensemble of a cooperative model for a device batch `image` [n,1,H,W]: the fast network's logits and the shape
    network's one refinement of them, stacked member-major -> [2n, C, H, W] (channels_last), for ops.predictive_stats(members=2).
    Eval mode, no gradients."""
    import torch
    from . import ops
    solver.eval()
    with torch.no_grad():
        _, first = solver.fast_predict(image)
        refined, _ = solver.slow_refinement(first, n_steps=1)
    return ops.as_nhwc(torch.cat([first.float(), refined.float()], dim=0))


# ---------------------------------------------------------------------------------------------- the test-time augmentation ensemble
def tta_members(solver, image, views, n_iter=None):
    """The T-member ensemble of a model over the D4 views `views` (tta.parse_views) of a device batch `image` [n,1,H,W]: every view's
    logits put back on the native grid, stacked member-major -> [T * n, C, H, W] (channels_last), for ops.predictive_stats(members=T).
    Two launches around one `predict` over the T * n stack (tta.predict_tta)."""
    from . import tta
    return tta.predict_tta(solver, image, views, n_iter=n_iter, want=("aligned",)).aligned
