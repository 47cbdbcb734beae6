"""Host statements of the supervised segmentation losses (medseg/models/custom_loss.py:8-40), float64 on the CPU: value and gradient of
every kind in closed form.  They are the definition the HIP kernels (csrc/ctl_loss.hip) are tested against, as prepare.py and corrupt.py
are for their stages; nothing on the training path calls them.

Notation: logits x[B,C,H,W], label map y[B,H,W], p = softmax(x, dim=C), t = onehot(y), M = B*H*W, s = 0.01.

  'cross entropy'           L = (1/M) sum_pix -log p_y                                                    (:706-740)
  'weighted cross entropy'  w' = w / sum(w) * C;  L = (1/M) sum_pix w'[y] * -log p_y (divisor M, not sum w');  dL/dx_k = w'[y] (p_k - t_k) / M.
                            class_weights=None is upstream's uniform 1/C, i.e. w' = 1: plain cross entropy.
  'dice', 'weighted dice'   per (b, k): I = sum_pix p t + s, U = sum_pix p + sum_pix t + s;  L = 1 - (sum_{b,k} 2I/U) / (B C)   (:356-396).
                            Upstream accepts `weight` and never uses it: 'weighted dice' IS 'dice'.
  'foreground dice'         classes 1..C-1: term (2 sum p t + s) / (sum p + sum t + s), divisor B (C-1); C = 1 is refused   (:434-471).
                            Both Dice forms: g_k = dL/dp_k = -(sel_k / div) (2 t_k / U - num / U^2), dL/dx_j = p_j (g_j - sum_k p_k g_k).
  'focal'                   L = (1/M) sum_pix -(1 - p_y)^gamma log p_y, gamma = 2 under this name (:222-255).  Upstream detaches p_y (:243):
                            the gradient is (1 - p_y)^gamma (p_k - t_k) / M, which is NOT the derivative of the value.
  'contour_smooth'          refused (upstream's own call raises TypeError).

A label outside 0..C-1 is no class: t = 0 for every k and weight 0 (upstream would fail on it).
`loss_type` may also be a mapping {name: weight}: sum of weight * L_name (no upstream counterpart; it exists for Dice + cross entropy)."""
from __future__ import annotations

from collections.abc import Mapping

import torch

SMOOTH = 0.01
LOSS_NAMES = ("cross entropy", "weighted cross entropy", "dice", "weighted dice", "foreground dice", "focal")


def parse_loss_type(loss_type, class_weights=None, num_classes=None):
    """[(name, weight)] of a loss name or a {name: weight} mapping, and the class weights as a tuple of floats (or None).  Unknown names and
    'contour_smooth' raise NotImplementedError; class weights of the wrong length, an empty mapping and 'foreground dice' of one class
    raise ValueError."""
    terms = [(k, float(v)) for k, v in loss_type.items()] if isinstance(loss_type, Mapping) else [(loss_type, 1.0)]
    for name, _ in terms:
        if name not in LOSS_NAMES:
            raise NotImplementedError(f"loss_type {name!r} (one of {', '.join(LOSS_NAMES)}, or a mapping of them to weights)")
    if not terms:
        raise ValueError("loss_type: empty mapping")
    if class_weights is not None:
        class_weights = tuple(float(v) for v in (class_weights.tolist() if hasattr(class_weights, "tolist") else class_weights))
        if num_classes is not None and len(class_weights) != num_classes:
            raise ValueError(f"each class must have a weight: expected {num_classes} weights, got {len(class_weights)}")
    if num_classes is not None and num_classes < 2 and any(n == "foreground dice" for n, _ in terms):
        raise ValueError("'foreground dice' needs at least 2 classes")
    return terms, class_weights


def normalised_weights(class_weights, c):
    """w' = w / sum(w) * C in float64 (custom_loss.py:733-734); None = upstream's uniform 1/C, i.e. ones."""
    if class_weights is None:
        return torch.ones(c, dtype=torch.float64)
    w = torch.as_tensor(class_weights, dtype=torch.float64).flatten()
    if w.numel() != c:
        raise ValueError(f"each class must have a weight: expected {c} weights, got {w.numel()}")
    total = float(w.sum())
    if not (total > 0.0 and total != float("inf")):
        raise ValueError(f"the class weights sum to {total}: a finite, positive sum is needed")
    return w / total * c


def _one(x, y, name, class_weights, gamma):
    b, c, h, w = x.shape
    m = b * h * w
    p, logp = torch.softmax(x, 1), torch.log_softmax(x, 1)
    t = (y.unsqueeze(1) == torch.arange(c).view(1, c, 1, 1)).double()
    if name in ("cross entropy", "weighted cross entropy", "focal"):
        if name == "focal":
            f = t.sum(1) * (1.0 - (p * t).sum(1)) ** gamma
        else:
            wn = normalised_weights(class_weights if name == "weighted cross entropy" else None, c)
            f = (t * wn.view(1, c, 1, 1)).sum(1)
        return (-f * (logp * t).sum(1)).sum() / m, f.unsqueeze(1) * (p - t) / m
    fg = name == "foreground dice"
    if fg and c < 2:
        raise ValueError("'foreground dice' needs at least 2 classes")
    sel = torch.ones(c, dtype=torch.float64)
    if fg:
        sel[0] = 0.0
    div = float(b * (c - 1 if fg else c))
    spt, u = (p * t).sum((2, 3)), p.sum((2, 3)) + t.sum((2, 3)) + SMOOTH
    num = 2.0 * spt + SMOOTH if fg else 2.0 * (spt + SMOOTH)
    g = -(sel.view(1, c, 1, 1) / div) * (2.0 * t / u[:, :, None, None] - (num / (u * u))[:, :, None, None])
    return 1.0 - (sel * num / u).sum() / div, p * (g - (p * g).sum(1, keepdim=True))


def loss_and_grad(logit, label, loss_type="cross entropy", class_weights=None, gamma=2.0, gout=1.0):
    """(loss, gout * dloss/dlogit), float64 CPU tensors (0-d and [B,C,H,W]) of a name or a {name: weight} mapping."""
    x, y = logit.detach().double().cpu(), label.detach().long().cpu()
    if x.dim() != 4 or y.shape != (x.shape[0], x.shape[2], x.shape[3]):
        raise ValueError("expected logits [B,C,H,W] and a label map [B,H,W]")
    terms, class_weights = parse_loss_type(loss_type, class_weights, x.shape[1])
    loss, grad = torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    for name, weight in terms:
        l, g = _one(x, y, name, class_weights, float(gamma))
        loss, grad = loss + weight * l, grad + weight * g
    return loss, grad * float(gout)


def loss_value(logit, label, loss_type="cross entropy", class_weights=None, gamma=2.0):
    return loss_and_grad(logit, label, loss_type, class_weights, gamma)[0]
