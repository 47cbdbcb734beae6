"""Image-similarity (reconstruction) losses between a prediction and a constant target image (medseg/models/custom_loss.py: smooth_l1_loss
:310-318, CustomNormalizedCrossCorrelationLoss :514-571, CustomLocalNormalizedCrossCorrelationLoss :574-661, next to the plain 'mse' / 'l1').

`similarity_and_grad` is the host statement, float64 on the CPU with the gradient in closed form: the definition the HIP kernels
(csrc/ctl_recon.hip) are tested against, as consistency.consistency_and_grad is for the consistency losses.  The public entries below it
carry upstream's names and arguments; device tensors go to the kernels, CPU tensors take the same arithmetic from plain torch ops.

Notation: prediction x[B,C,H,W]; target t of the same shape or [1,C,H,W] (upstream's single template, broadcast over the batch), a
constant; optional per-pixel mask m[B,1,H,W] or [B,H,W] of any dtype, nonzero -> 1, which multiplies x and t BEFORE anything else
(J = m x, I = m t, upstream's `image * mask`).  N = B C H W; reduction 'mean' or 'sum'.  Every gradient is dL/dx = m dL/dJ.

  'mse'        (1/N) sum (J - I)^2 ('sum': without the 1/N, likewise below);  dL/dJ = 2 (J - I) / N.
  'l1'         (1/N) sum |J - I|;  dL/dJ = sign(J - I) / N, 0 where they are equal.
  'smooth l1'  (1/N) sum f(|J - I|) with f(n) = 0.5 n^2 / beta where n < beta, else n - 0.5 beta (:313-315), beta > 0;
               dL/dJ = ((J - I) / beta where n < beta, else sign(J - I)) / N.
  'ncc'        1 - (1/B) sum_b s_b ('sum': 1 - sum_b s_b).  With zero_mean, a = J - mean_{H,W} J and u = I - mean_{H,W} I per sample AND
               channel (:545-549), else a = J, u = I.  Per sample, over all C H W elements, with eps = 1e-6:
                   s_b = <a, u> / (max(|a|, eps) max(|u|, eps)),
               which is what the installed torch's nn.CosineSimilarity(dim=1, eps=1e-6) computes: each norm is clamped from below by eps on
               its own (not their product, as torch < 1.12 did), so s_b = 0 for a constant plane under zero_mean.  The gradient is that
               of this formula: ds_b/da = u / (Na Nu) - [|a| > eps] <a, u> a / (Na^3 Nu) with Na = max(|a|, eps), Nu = max(|u|, eps); the
               mean subtraction adds nothing to it (both u and a sum to zero over a plane).
  'lncc'       1 - (1/N) sum_p score_p ('sum': 1 - sum_p score_p), upstream's ncc (:608-661) with win odd, 3 <= win <= 15, win <= H, W.
               The five window sums I_sum, J_sum, I2_sum, J2_sum, IJ_sum are taken with zero padding win // 2 over the win x win window AND
               OVER ALL C CHANNELS (upstream's all-ones C x C filter), so the score map has C identical channels, and A = win^2 whatever C
               is (the padding zeros and the other channels are counted in the sums but not in A).  With uI = I_sum / A, uJ = J_sum / A:
                   cross = IJ_sum - uJ I_sum - uI J_sum + uI uJ A,  I_var = I2_sum - 2 uI I_sum + uI^2 A,  J_var likewise,
                   D = sqrt(I_var) sqrt(J_var) + 1e-6,  score = cross / D.
               d score_p / dJ_q = a_p (I_q - uI_p) - b_p (J_q - uJ_p) for q in the window of p, a_p = 1 / D_p,
               b_p = cross_p sqrt(I_var_p) / (D_p^2 sqrt(J_var_p)), so
                   dL/dJ_q = -(C/N) (I_q Sa - J_q Sb + Sc),  Sa, Sb, Sc = the window sums of a, b and b uJ - a uI over the centres p
               whose window contains q ('sum': the factor is C; the C identical score channels each count).
               FLAT RULE (a deviation from upstream that makes the loss a function): a variance is flat when var <= 2^-40 (its sum of
               squares); this includes every negative round-off value, a NaN upstream.  A flat variance counts as exactly 0, and the b_p of
               a flat J_var is 0, where upstream's autograd gives inf * 0.  Windows whose ratio var / (sum of squares) lies in
               (2^-44, 2^-36) are FLAGGED: a different summation order could fall on the other side of the rule there.

`kinds` is a name, a sequence of names with `weights`, or a {name: weight} mapping; the total is the weighted sum."""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _ffi      # the kind constants only: the library itself is loaded by the first call into it
from .losses import MAX_CLASSES, check_constant, check_mask, check_names, mask01

# the names (custom_loss.py:310-318, :514-571, :574-661) -> CTL_RECON_* bit; bit k is kind k, the order of the terms and of the weights
RECON_KINDS = {"mse": _ffi.RECON_MSE, "l1": _ffi.RECON_L1, "smooth l1": _ffi.RECON_SMOOTH_L1, "ncc": _ffi.RECON_NCC, "lncc": _ffi.RECON_LNCC}
RECON_NAMES = tuple(RECON_KINDS)
MAX_CHANNELS = MAX_CLASSES
EPS = 1e-6
FLAT_RATIO, FLAG_LO, FLAG_HI = 2.0 ** -40, 2.0 ** -44, 2.0 ** -36

# loss, grad: the weighted total (0-d) and gout * dloss/dx [B,C,H,W]; terms / grads: {name: ...} at unit weight and gout = 1; flagged: the
# number of flagged windows (0 without 'lncc'); lncc: None or a dict of per-centre maps [B,H,W] (score, D, sqrt_I_var, sqrt_J_var, cross,
# the five sums, flat_I, flat_J, flagged) from which a test evaluates the sensitivities 1 / D_p and 1 / sqrt(J_var_p)
Similarity = namedtuple("Similarity", "loss grad terms grads flagged lncc")


def parse_kinds(kinds, weights=None):
    """{name: weight} of a name, a sequence of names (with `weights`, default ones) or a mapping.  Unknown names: NotImplementedError."""
    if isinstance(kinds, str):
        kinds = [kinds]
    if isinstance(kinds, dict):
        if weights is not None:
            raise ValueError("`weights` cannot be given next to a {name: weight} mapping")
        names, weights = list(kinds), list(kinds.values())
    else:
        names = list(kinds)
        weights = [1.0] * len(names) if weights is None else ([weights] if isinstance(weights, (int, float)) else list(weights))
    if len(names) != len(weights):
        raise ValueError(f"kinds and weights: {len(names)} names, {len(weights)} weights (the same number)")
    check_names(names, RECON_KINDS, "image-similarity loss")
    out = {}
    for name, weight in zip(names, weights):
        weight = float(weight)
        if weight != weight or weight in (float("inf"), float("-inf")):
            raise ValueError(f"the weight of {name!r} is {weight} (finite)")
        out[name] = out.get(name, 0.0) + weight
    return out


def check_win(win):
    if int(win) != win or win % 2 == 0 or not 3 <= win <= 15:
        raise ValueError(f"win = {win} (the window size win_size: odd, 3 .. 15)")


def check_params(names, beta=1.0 / 9, win=9, reduction="mean", device=False):
    """ValueError for a parameter no kernel takes, of the kinds `names` only; checked before any tensor is looked at.  device: the
    kernels do not offer reduction='none' (NotImplementedError), which only the CPU path of image_similarity takes."""
    if device and reduction == "none":
        raise NotImplementedError("reduction='none' is not offered on the device ('mean' or 'sum'; CPU tensors take 'none')")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction {reduction!r} ('mean' or 'sum')")
    if "smooth l1" in names and not float(beta) > 0.0:
        raise ValueError(f"beta = {beta} (smooth l1 needs beta > 0)")
    if "lncc" in names:
        check_win(win)


def check_image(names, shape, win=9):
    """ValueError for an image [B,C,H,W] the kernels do not take: its channel count, and a plane smaller than the window of 'lncc'."""
    _, c, h, w = shape
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"{c} channels (1 .. {MAX_CHANNELS})")
    if "lncc" in names and (win > h or win > w):
        raise ValueError(f"win = {win} is larger than the {h}x{w} plane (window size must not exceed the image dimension)")


def check_pair(x, t, mask=None):
    if x.dim() != 4 or t.dim() != 4 or tuple(t.shape[1:]) != tuple(x.shape[1:]) or t.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"expected a prediction [B,C,H,W] and a target of that shape or [1,C,H,W], got {tuple(x.shape)} and {tuple(t.shape)}")
    check_constant(t, "target")
    check_mask(mask, x.shape)


def box_sum(v, win):
    """The zero-padded win x win window sum of every plane of v[...,H,W]: rows first, then columns, each in index order."""
    r = win // 2
    h, w = v.shape[-2:]
    z = F.pad(v, (r, r, 0, 0))
    rows = z[..., :, 0:w].clone()
    for k in range(1, win):
        rows = rows + z[..., :, k:k + w]
    z = F.pad(rows, (0, 0, r, r))
    out = z[..., 0:h, :].clone()
    for k in range(1, win):
        out = out + z[..., k:k + h, :]
    return out


def lncc_maps(I, J, win):
    """Per-centre maps [B,H,W] of 'lncc' for masked I (target) and J (prediction), float64: see Similarity.lncc."""
    A = float(win * win)
    sums = {k: box_sum(v.sum(1), win) for k, v in (("I_sum", I), ("J_sum", J), ("I2_sum", I * I), ("J2_sum", J * J), ("IJ_sum", I * J))}
    uI, uJ = sums["I_sum"] / A, sums["J_sum"] / A
    cross = sums["IJ_sum"] - uJ * sums["I_sum"] - uI * sums["J_sum"] + uI * uJ * A
    I_var = sums["I2_sum"] - 2.0 * uI * sums["I_sum"] + uI * uI * A
    J_var = sums["J2_sum"] - 2.0 * uJ * sums["J_sum"] + uJ * uJ * A
    flat_I, flat_J = I_var <= FLAT_RATIO * sums["I2_sum"], J_var <= FLAT_RATIO * sums["J2_sum"]
    flagged = torch.zeros_like(flat_I)
    for var, sq in ((I_var, sums["I2_sum"]), (J_var, sums["J2_sum"])):
        flagged |= (var > FLAG_LO * sq) & (var < FLAG_HI * sq)
    sI = torch.where(flat_I, torch.zeros_like(I_var), I_var.clamp_min(0.0).sqrt())
    sJ = torch.where(flat_J, torch.zeros_like(J_var), J_var.clamp_min(0.0).sqrt())
    D = sI * sJ + EPS
    out = dict(sums, uI=uI, uJ=uJ, cross=cross, sqrt_I_var=sI, sqrt_J_var=sJ, D=D, score=cross / D, flat_I=flat_I, flat_J=flat_J, flagged=flagged)
    return out


def _one(name, I, J, m, beta, win, zero_mean, mean):
    """(loss, dloss/dx, lncc maps or None) of one kind at unit weight; float64, I / J masked, m[B,1,H,W] of 0/1.  The value of a pointwise
    kind is `_value`, the function the CPU path differentiates; the gradient is the closed form of the module docstring."""
    b, c, h, w = J.shape
    d = J - I
    if name in ("mse", "l1", "smooth l1"):
        div = float(b * c * h * w) if mean else 1.0
        g = 2.0 * d if name == "mse" else torch.sign(d) if name == "l1" else torch.where(d.abs() < beta, d / beta, torch.sign(d))
        return _value(name, I, J, beta, win, zero_mean, "mean" if mean else "sum"), m * g / div, None
    if name == "ncc":
        a, u = (J - J.mean((2, 3), keepdim=True), I - I.mean((2, 3), keepdim=True)) if zero_mean else (J, I)
        dot = (a * u).sum((1, 2, 3))
        na, nu = (a * a).sum((1, 2, 3)).sqrt(), (u * u).sum((1, 2, 3)).sqrt()
        Na, Nu = na.clamp_min(EPS), nu.clamp_min(EPS)
        s = dot / (Na * Nu)             # its own statement: the norm() of `_ncc_scores_torch` rounds differently
        alpha = 1.0 / (Na * Nu)
        bet = torch.where(na > EPS, dot / (Na ** 3 * Nu), torch.zeros_like(dot))
        div = float(b) if mean else 1.0
        g = alpha.view(b, 1, 1, 1) * u - bet.view(b, 1, 1, 1) * a
        return 1.0 - s.sum() / div, -m * g / div, None
    # 'lncc' keeps two statements of its value as well: box_sum in index order is the definition, the conv2d form of `_value` is the CPU
    # path, and the two round differently
    mp = lncc_maps(I, J, win)
    a_p = 1.0 / mp["D"]
    b_p = torch.where(mp["flat_J"], torch.zeros_like(a_p),
                      mp["cross"] * mp["sqrt_I_var"] / (mp["D"] * mp["D"] * torch.where(mp["flat_J"], torch.ones_like(a_p), mp["sqrt_J_var"])))
    c_p = b_p * mp["uJ"] - a_p * mp["uI"]
    Sa, Sb, Sc = (box_sum(v, win).unsqueeze(1) for v in (a_p, b_p, c_p))
    fac = (1.0 / float(b * h * w)) if mean else float(c)          # C identical score channels: C / N = 1 / (B H W)
    mp = dict(mp, a=a_p, b=b_p)
    return 1.0 - fac * mp["score"].sum(), -fac * m * (I * Sa - J * Sb + Sc), mp


def similarity_and_grad(x, t, kinds, weights=None, mask=None, *, beta=1.0 / 9, win=9, zero_mean=True, reduction="mean", gout=1.0):
    """The definition (module docstring): a `Similarity` of float64 CPU tensors, the gradient with respect to x in closed form."""
    terms = parse_kinds(kinds, weights)
    check_params(terms, beta, win, reduction)
    check_pair(x, t, mask)
    check_image(terms, x.shape, win)
    xd = x.detach().double().cpu()
    td = t.detach().double().cpu().expand_as(xd)
    m = mask01(None if mask is None else mask.cpu(), xd.shape, torch.float64, "cpu")
    I, J = td * m, xd * m
    loss, grad = torch.zeros((), dtype=torch.float64), torch.zeros_like(xd)
    values, grads, maps = {}, {}, None
    for name, weight in terms.items():
        l, g, mp = _one(name, I, J, m, float(beta), int(win), bool(zero_mean), reduction == "mean")
        values[name], grads[name] = l, g
        maps = mp if mp is not None else maps
        loss, grad = loss + weight * l, grad + weight * g
    flagged = 0 if maps is None else int(maps["flagged"].sum())
    return Similarity(loss, grad * float(gout), values, grads, flagged, maps)


# ---------------------------------------------------------------------------------------------- the values from differentiable torch ops
def _lncc_scores_torch(I, J, win):
    """score [B,1,H,W] from differentiable torch ops in J's dtype, the flat rule included (a flat variance: 0, and no gradient through it)"""
    A = float(win * win)
    k = torch.ones(1, 1, win, win, dtype=J.dtype, device=J.device)
    box = lambda v: F.conv2d(v.sum(1, keepdim=True), k, padding=win // 2)      # noqa: E731
    I_sum, J_sum, I2_sum, J2_sum, IJ_sum = box(I), box(J), box(I * I), box(J * J), box(I * J)
    uI, uJ = I_sum / A, J_sum / A
    cross = IJ_sum - uJ * I_sum - uI * J_sum + uI * uJ * A
    I_var = I2_sum - 2 * uI * I_sum + uI * uI * A
    J_var = J2_sum - 2 * uJ * J_sum + uJ * uJ * A

    def root(var, sq):
        flat = var <= FLAT_RATIO * sq
        return torch.where(flat, torch.zeros_like(var), torch.where(flat, torch.ones_like(var), var).sqrt())

    return cross / (root(I_var, I2_sum) * root(J_var, J2_sum) + EPS)


def _ncc_scores_torch(I, J, zero_mean):
    if zero_mean:
        I, J = I - I.mean((2, 3), keepdim=True), J - J.mean((2, 3), keepdim=True)
    b = J.shape[0]
    a, u = J.reshape(b, -1), I.reshape(b, -1)
    na, nu = a.norm(dim=1), u.norm(dim=1)
    return (a * u).sum(1) / (torch.where(na > EPS, na, torch.full_like(na, EPS)) * nu.clamp_min(EPS))


def _value(name, I, J, beta, win, zero_mean, reduction):
    """One kind at unit weight between the masked target I and prediction J, in J's dtype; reduction 'none' gives its unreduced form."""
    red = (lambda v: v.mean()) if reduction == "mean" else (lambda v: v.sum()) if reduction == "sum" else (lambda v: v)
    d = J - I
    if name == "mse":
        return red(d * d)
    if name == "l1":
        return red(d.abs())
    if name == "smooth l1":
        n = d.abs()
        return red(torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta))
    if name == "ncc":
        s = _ncc_scores_torch(I, J, zero_mean)
        return 1.0 - (s.sum() / float(J.shape[0]) if reduction == "mean" else s.sum() if reduction == "sum" else s)
    return 1.0 - red(_lncc_scores_torch(I, J, win).expand(-1, J.shape[1], -1, -1))


def _similarity_torch(x, t, terms, mask, beta, win, zero_mean, reduction):
    """The weighted total (or, reduction 'none' with a single kind, its unreduced form) from torch ops in x's float dtype."""
    x = x if x.is_floating_point() else x.float()
    t = t.detach().to(x.dtype).expand_as(x)
    m = mask01(mask, x.shape, x.dtype, x.device)
    I, J = t * m, x * m
    total = 0.0
    for name, weight in terms.items():
        total = total + weight * _value(name, I, J, beta, win, zero_mean, reduction)
    return total


def image_similarity(x, t, kinds, weights=None, mask=None, *, beta=1.0 / 9, win=9, zero_mean=True, reduction="mean"):
    """The weighted sum of the image-similarity losses of RECON_NAMES, differentiable in x (a 0-d tensor).  Device tensors run the HIP
    kernels (fp32); CPU tensors take the same arithmetic from torch ops in their own float dtype.  `reduction='none'` (one kind, CPU
    tensors only) returns the unreduced form; on the device it raises NotImplementedError."""
    terms = parse_kinds(kinds, weights)
    device = x.is_cuda or t.is_cuda
    if reduction == "none" and not device:
        if len(terms) != 1:
            raise ValueError("reduction='none' takes a single kind")
        check_params(terms, beta, win, "mean")
    else:
        check_params(terms, beta, win, reduction, device)
    check_pair(x, t, mask)
    check_image(terms, x.shape, win)
    if not device:
        return _similarity_torch(x, t, terms, mask, float(beta), int(win), bool(zero_mean), reduction)
    from . import autograd
    return autograd.image_similarity_loss(x, t.detach(), terms, None, mask, beta=beta, win=win, zero_mean=zero_mean, reduction=reduction)


# ---------------------------------------------------------------------------------------------- upstream's names
def smooth_l1_loss(input, target, beta=1. / 9, size_average=True):
    """custom_loss.py:310-318."""
    return image_similarity(input, target, "smooth l1", beta=beta, reduction="mean" if size_average else "sum")


class CustomNormalizedCrossCorrelationLoss(nn.Module):
    """custom_loss.py:514-571: 1 - the (zero-normalised) cross-correlation of `image` [B,C,H,W] with `template` ([1,C,H,W], or one per
    sample).  Differentiable in `image`; the template is a constant.  `use_gpu` is kept for the signature: the tensors decide."""

    def __init__(self, use_gpu=True, reduction='mean', zero_mean=False):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise NotImplementedError(f"reduction {reduction!r} ('mean', 'sum' or 'none')")
        self.use_gpu, self.epsilon, self.reduction, self.zero_mean = use_gpu, EPS, reduction, zero_mean

    def forward(self, template, image):
        return image_similarity(image, template, "ncc", zero_mean=self.zero_mean, reduction=self.reduction)


class CustomLocalNormalizedCrossCorrelationLoss(nn.Module):
    """custom_loss.py:574-661: 1 - the local (sliding window) normalised cross-correlation, the module docstring's 'lncc'."""

    def __init__(self, win_size=9, use_gpu=True, reduction='mean'):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise NotImplementedError(f"reduction {reduction!r} ('mean', 'sum' or 'none')")
        check_win(win_size)
        self.use_gpu, self.epsilon, self.reduction, self.win_size = use_gpu, EPS, reduction, int(win_size)

    def forward(self, template, image, mask=None):
        return image_similarity(image, template, "lncc", mask=mask, win=self.win_size, reduction=self.reduction)
