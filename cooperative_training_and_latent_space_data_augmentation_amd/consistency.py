"""Consistency losses between two PREDICTIONS (medseg/models/custom_loss.py: calc_segmentation_consistency :892-973, kl_divergence :863-889,
soft-target cross_entropy_2D :741-766, the softmax 'mse' :942-952, SoftDiceLoss with a 4-D target :356-396, the Sobel contour_loss :784-860).

`consistency_and_grad` is the host statement, float64 on the CPU with the gradient in closed form: the definition the HIP kernels
(csrc/ctl_consist.hip) are tested against, as losses.loss_and_grad is for the supervised losses.  The public functions below it carry
upstream's names and arguments; device tensors go to the kernels, CPU tensors take the same arithmetic from plain torch ops.

Notation: output logits x[B,C,H,W], reference r[B,C,H,W]; q = softmax(x); p = softmax(r), or p = r when is_gt.  Optional per-pixel mask
m[B,1,H,W] or [B,H,W] of any dtype, nonzero -> 1.  M = B*H*W, R = sum m (M without a mask), s = 0.01.  The reference is a constant.

  'kl'           (1/M) sum_pix m sum_k p_k (log p_k - log q_k); the divisor is M with or without a mask.  With is_gt upstream's rule, kept:
                 p_k = 1.0 where r_k != 0, else float32(1e-8) = 9.99999993922529e-09, and p_k log p_k = 0 resp. the float32 product
                 float32(1e-8) * log(float32(1e-8)).  Soft targets are binarised by it and S = sum_k p_k != 1.
                 dL/dx_j = (m/M)(S q_j - p_j).
  'ce'           -(1/R) sum_pix m sum_k w'_k p_k log q_k with w' = 1;  R = 0 gives loss 0 and a zero gradient.
  'weighted ce'  the same with w' = w / sum(w) * C (losses.normalised_weights); without class_weights: ValueError.
                 dL/dx_j = (m/R)(q_j sum_k w'_k p_k - w'_j p_j).
  'mse'          (1/M) sum_pix m sum_k (q_k - p_k)^2;  g_k = 2 m (q_k - p_k) / M,  dL/dx_j = q_j (g_j - sum_k q_k g_k).
  'Dice'         1 - (sum_{b,k} 2I/U) / (B C);  per (b,k): I = sum m q p + s,  U = sum m q + sum m p + s;
                 g_k = -(m / (B C)) (2 p_k / U - 2 I / U^2), then the softmax Jacobian as for 'mse'.
  'contour'      (1/(C-1)) sum_{k=1..C-1} 1/2 (1/M) sum_pix m (E_x^2 + E_y^2), C >= 2 (else ValueError).  With d = q - p: E_x, E_y are the 3x3
                 zero-padded cross-correlations of d_k with S_x = [[1,0,-1],[2,0,-2],[1,0,-1]] and S_y = [[1,2,1],[0,0,0],[-1,-2,-1]]
                 (:823-841; the filter is linear, so G(q) - G(p) = G(d)).  g_k = (1/((C-1) M)) (S_x^T(m E_x) + S_y^T(m E_y))_k, g_0 = 0,
                 then the softmax Jacobian as for 'mse'.

The total is (1/len(scales)) sum_s 2^s sum_t weight_t L_t(pool_s x, pool_s r) with pool_s = AvgPool2d(2^s): window = stride = 2^s, floor
sizes, 0 <= s <= 4.  A plane smaller than the window, and a mask together with any s > 0, raise ValueError.  Unknown names raise
NotImplementedError, as upstream does; reference.requires_grad raises ValueError (upstream lets gradients reach the reference)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _ffi      # the kind constants only: the library itself is loaded by the first call into it
from .losses import SMOOTH, check_constant, check_mask, check_names, check_two_classes, class_weight_tuple, mask01, normalised_weights

# names of calc_segmentation_consistency (custom_loss.py:892-973) -> CTL_CONS_* bit; bit t is kind t, the order of the terms and of the weights
CONSISTENCY_KINDS = {"kl": _ffi.CONS_KL, "ce": _ffi.CONS_CE, "weighted ce": _ffi.CONS_WCE, "mse": _ffi.CONS_MSE, "Dice": _ffi.CONS_DICE,
                     "contour": _ffi.CONS_CONTOUR}
CONSISTENCY_NAMES = tuple(CONSISTENCY_KINDS)
MAX_SCALE = 4
_P8_T = torch.tensor(1e-8, dtype=torch.float32)
P8 = float(_P8_T)                                   # upstream's torch.where(reference == 0, 1e-8, 1 - 1e-8) is a float32 tensor: 1e-8 and 1.0
P8_LOG_P8 = float(_P8_T * torch.log(_P8_T))         # its p log p, a float32 product


def parse_consistency(divergence_types, divergence_weights, class_weights, scales, mask, num_classes):
    """([(name, weight)], normalised class weights or None, [scale]).  Raises what the module docstring says."""
    names = [divergence_types] if isinstance(divergence_types, str) else list(divergence_types)
    weights = [divergence_weights] if isinstance(divergence_weights, (int, float)) else list(divergence_weights)
    if len(names) != len(weights):
        raise ValueError(f"divergence_types and divergence_weights: {len(names)} names, {len(weights)} weights (the same number)")
    check_kinds(names, class_weights)
    if "contour" in names:
        check_two_classes("contour", num_classes)
    wn = None if class_weights is None else normalised_weights(class_weights, num_classes)
    scales = [scales] if isinstance(scales, int) else list(scales)
    if not scales or any(int(s) != s or not 0 <= s <= MAX_SCALE for s in scales):
        raise ValueError(f"scales {scales}: a non-empty list of integers 0 .. {MAX_SCALE}")
    if mask is not None and any(s > 0 for s in scales):
        raise ValueError("a mask cannot be combined with a scale above 0 (the mask is not pooled)")
    return [(n, float(w)) for n, w in zip(names, weights)], wn, [int(s) for s in scales]


def check_kinds(names, class_weights):
    """The names and what they need of the other arguments: checked before any tensor is looked at."""
    check_names(names, CONSISTENCY_KINDS, "consistency loss")
    if "weighted ce" in names and class_weights is None:
        raise ValueError("'weighted ce' must be given class weights")


def check_pair(output, reference, mask=None):
    """Shapes of the two predictions and of the mask; the reference must not require grad."""
    if output.dim() != 4 or tuple(output.shape) != tuple(reference.shape):
        raise ValueError(f"expected output and reference logits of one shape [B,C,H,W], got {tuple(output.shape)} and {tuple(reference.shape)}")
    check_constant(reference, "reference")
    check_mask(mask, output.shape)


def check_plane(h, w, scale):
    if (h >> scale) < 1 or (w >> scale) < 1:
        raise ValueError(f"a {h}x{w} plane is smaller than the {1 << scale}x{1 << scale} window of scale {scale}")


def _pad_shifts(d):
    h, w = d.shape[-2:]
    z = F.pad(d, (1, 1, 1, 1))
    return lambda a, b: z[..., a:a + h, b:b + w]           # the value at (i + a - 1, j + b - 1), zero outside the plane


def sobel(d):
    """(E_x, E_y): the zero-padded 3x3 cross-correlations of every plane of d[...,H,W] with S_x and S_y."""
    s = _pad_shifts(d)
    ex = s(0, 0) - s(0, 2) + 2.0 * (s(1, 0) - s(1, 2)) + s(2, 0) - s(2, 2)
    ey = s(0, 0) + 2.0 * s(0, 1) + s(0, 2) - s(2, 0) - 2.0 * s(2, 1) - s(2, 2)
    return ex, ey


def sobel_t(ex, ey):
    """S_x^T ex + S_y^T ey: the transposes of the two maps of `sobel`."""
    sx, sy = _pad_shifts(ex), _pad_shifts(ey)
    gx = sx(2, 2) - sx(2, 0) + 2.0 * (sx(1, 2) - sx(1, 0)) + sx(0, 2) - sx(0, 0)
    gy = sy(2, 2) + 2.0 * sy(2, 1) + sy(2, 0) - sy(0, 2) - 2.0 * sy(0, 1) - sy(0, 0)
    return gx + gy


def pool(x, scale):
    """AvgPool2d(2^scale) of [B,C,H,W]: floor sizes."""
    if scale == 0:
        return x
    b, c, h, w = x.shape
    check_plane(h, w, scale)
    k, ho, wo = 1 << scale, h >> scale, w >> scale
    return x[:, :, :ho * k, :wo * k].reshape(b, c, ho, k, wo, k).sum((3, 5)) / float(k * k)


def unpool(g, scale, h, w):
    """The transpose of `pool`: g * 4^-scale on every pixel of a window, zero on the rows and columns the floor drops."""
    if scale == 0:
        return g
    k = 1 << scale
    out = g.new_zeros(g.shape[:2] + (h, w))
    out[:, :, :g.shape[2] * k, :g.shape[3] * k] = g.repeat_interleave(k, 2).repeat_interleave(k, 3) / float(k * k)
    return out


def _through_softmax(q, g):
    return q * (g - (q * g).sum(1, keepdim=True))


def _one(x, r, name, wn, m, is_gt):
    """(loss, grad) of one kind at one scale, m[B,1,H,W] of 0/1, in x's dtype: the value from differentiable torch ops (the CPU path takes
    it as it is) and grad() = dloss/dx in closed form, which the host statement evaluates."""
    b, c, h, w = x.shape
    M = float(b * h * w)
    q, logq = torch.softmax(x, 1), torch.log_softmax(x, 1)
    if name == "kl":
        if is_gt:
            nz = r != 0
            p = torch.where(nz, torch.ones_like(r), torch.full_like(r, P8))
            plogp = torch.where(nz, torch.zeros_like(r), torch.full_like(r, P8_LOG_P8))
        else:
            p = torch.softmax(r, 1)
            plogp = p * torch.log_softmax(r, 1)
        return (m * (plogp - p * logq)).sum() / M, lambda: (m / M) * (p.sum(1, keepdim=True) * q - p)
    p = r if is_gt else torch.softmax(r, 1)
    if name in ("ce", "weighted ce"):
        wv = (torch.ones(c, dtype=x.dtype, device=x.device) if name == "ce" else wn.to(device=x.device, dtype=x.dtype)).view(1, c, 1, 1)
        R = float(m.sum())
        if R == 0.0:
            return (x * 0.0).sum(), lambda: torch.zeros_like(x)
        return -(m * wv * p * logq).sum() / R, lambda: (m / R) * (q * (wv * p).sum(1, keepdim=True) - wv * p)
    if name == "mse":
        return (m * (q - p) ** 2).sum() / M, lambda: _through_softmax(q, 2.0 * m * (q - p) / M)
    if name == "Dice":
        inter = (m * q * p).sum((2, 3), keepdim=True) + SMOOTH
        union = (m * q).sum((2, 3), keepdim=True) + (m * p).sum((2, 3), keepdim=True) + SMOOTH
        return 1.0 - (2.0 * inter / union).sum() / float(b * c), \
            lambda: _through_softmax(q, -(m / float(b * c)) * (2.0 * p / union - 2.0 * inter / (union * union)))
    ex, ey = sobel((q - p)[:, 1:])

    def contour_grad():
        g = torch.zeros_like(x)
        g[:, 1:] = sobel_t(m * ex, m * ey) / (float(c - 1) * M)
        return _through_softmax(q, g)
    return 0.5 * (m * (ex * ex + ey * ey)).sum() / (float(c - 1) * M), contour_grad


def consistency_and_grad(output, reference, divergence_types=("kl", "contour"), divergence_weights=(1.0, 0.5), class_weights=None,
                         scales=(0,), mask=None, is_gt=False, gout=1.0):
    """(loss, gout * dloss/doutput): float64 CPU tensors (0-d and [B,C,H,W]), the gradient in closed form."""
    check_pair(output, reference, mask)
    x, r = output.detach().double().cpu(), reference.detach().double().cpu()
    terms, wn, scales = parse_consistency(divergence_types, divergence_weights, class_weights, scales, mask, x.shape[1])
    m = mask01(None if mask is None else mask.cpu(), x.shape, torch.float64, "cpu")
    loss, grad = torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    for s in scales:
        xs, rs = pool(x, s), pool(r, s)
        ms = m if s == 0 else torch.ones((xs.shape[0], 1) + tuple(xs.shape[2:]), dtype=torch.float64)
        for name, weight in terms:
            l, g = _one(xs, rs, name, wn, ms, bool(is_gt))
            loss = loss + float(1 << s) * weight * l
            grad = grad + float(1 << s) * weight * unpool(g(), s, x.shape[2], x.shape[3])
    n = float(len(scales))
    return loss / n, grad * (float(gout) / n)


# ---------------------------------------------------------------------------------------------- the CPU path of the public functions
def _consistency_torch(output, reference, terms, wn, scales, mask, is_gt):
    x = output if output.is_floating_point() else output.float()
    r = reference.detach().to(x.dtype)
    m = mask01(mask, x.shape, x.dtype, x.device)
    total = 0.0
    for s in scales:
        xs, rs = pool(x, s), pool(r, s)
        ms = m if s == 0 else torch.ones((xs.shape[0], 1) + tuple(xs.shape[2:]), dtype=x.dtype, device=x.device)
        for name, weight in terms:
            total = total + float(1 << s) * weight * _one(xs, rs, name, wn, ms, is_gt)[0]
    return total / float(len(scales))


# ---------------------------------------------------------------------------------------------- upstream's names
def calc_segmentation_consistency(output, reference, divergence_types=("kl", "contour"), divergence_weights=(1.0, 0.5), class_weights=None,
                                  scales=(0,), mask=None, is_gt=False):
    """custom_loss.py:892-973 as the module docstring states it (without the print): a 0-d tensor, differentiable in `output`.  Device
    tensors run the HIP kernels (fp32); CPU tensors take the same arithmetic from torch ops in their own float dtype."""
    check_pair(output, reference, mask)
    terms, wn, scales = parse_consistency(divergence_types, divergence_weights, class_weights, scales, mask, output.shape[1])
    for s in scales:
        check_plane(output.shape[2], output.shape[3], s)
    if not (output.is_cuda or reference.is_cuda):
        return _consistency_torch(output, reference, terms, wn, scales, mask, bool(is_gt))
    from . import autograd, ops
    ops.require_gpu(output, reference, mask)
    kinds = {}
    for name, weight in terms:
        kinds[name] = kinds.get(name, 0.0) + weight
    class_weights = class_weight_tuple(class_weights)
    reference = reference.detach()
    if scales == [0]:
        return autograd.consistency_loss(output, reference, kinds, class_weights, mask, bool(is_gt))
    total = None
    for s in scales:
        xs = autograd.avg_pool(output, s) if s else output
        rs = ops.avgpool_fwd(ops.as_nhwc(reference), s) if s else reference
        term = autograd.consistency_loss(xs, rs, kinds, class_weights, mask if s == 0 else None, bool(is_gt)) * float(1 << s)
        total = term if total is None else total + term
    return total / float(len(scales))


def kl_divergence(reference, pred, mask=None, is_gt=False):
    """custom_loss.py:863-889: KL(p || q) of the reference p and the prediction q (both logits; is_gt: the module docstring's rule)."""
    return calc_segmentation_consistency(pred, reference, ["kl"], [1.0], mask=mask, is_gt=is_gt)


def calc_segmentation_mse_consistency(input, target):
    return calc_segmentation_consistency(output=input, reference=target, divergence_types=["mse"], divergence_weights=[1.0])


def calc_segmentation_kl_consistency(input, target):
    return calc_segmentation_consistency(output=input, reference=target, divergence_types=["kl"], divergence_weights=[1.0])
