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

Distance-map losses (no upstream counterpart; kernels in csrc/ctl_dist.hip and csrc/ctl_loss.hip).  For a class k let S be the pixels of a
slice with y == k (a label outside 0..C-1 belongs to no S).  The class field F_k(p) is a Euclidean distance in pixels within the slice: for
p outside S to the nearest pixel of S, for p inside S to the nearest pixel not in S, i.e. distance_transform_edt(~S) + distance_transform_edt(S)
when both sets are non-empty; F_k = 0 everywhere if S is empty or fills the plane.  D2_k = F_k^2 is an exact integer.  The signed map
(Kervadec's one_hot2dist) is phi_k = F_k outside S and -(F_k - 1) inside, 0 where F_k = 0.  The confident label of a prediction is q = k where
softmax(x)_k > 0.5 (strictly; at most one class qualifies), else 255.  Classes 1..C-1, div = B (C-1) H W, C >= 2:
  'boundary'                L = (1/div) sum p_k phi_k (Kervadec et al., MIDL 2019);  g_k = phi_k / div, g_0 = 0.  Negative for a good prediction.
  'hausdorff dt'            L = (1/div) sum (p_k - t_k)^2 (D2t_k + D2p_k) (Karimi & Salcudean, IEEE TMI 2019, alpha = 2) with D2t the squared
                            field of y and D2p that of the confident label of x, a constant;  g_k = 2 (p_k - t_k)(D2t_k + D2p_k) / div, g_0 = 0.
                            Both: dL/dx_j = p_j (g_j - sum_k p_k g_k).

A label outside 0..C-1 is no class: t = 0 for every k and weight 0 (upstream would fail on it).
`loss_type` may also be a mapping {name: weight}: sum of weight * L_name (no upstream counterpart; it exists for Dice + cross entropy)."""
from __future__ import annotations

from collections.abc import Mapping

import torch

from . import _ffi      # the kind constants only: the library itself is loaded by the first call into it

SMOOTH = 0.01
# names of basic_loss_fn (custom_loss.py:8-40) -> CTL_LOSS_* kind of the fused kernels; upstream's 'weighted dice' never uses its weights: it
# is 'dice'.  'cross entropy' is a name without a fused kind (it has its own kernel pair, ops.ce2d_fwd / ce2d_bwd).
LOSS_KINDS = {"weighted cross entropy": _ffi.LOSS_WCE, "focal": _ffi.LOSS_FOCAL, "dice": _ffi.LOSS_DICE, "weighted dice": _ffi.LOSS_DICE,
              "foreground dice": _ffi.LOSS_FG_DICE}
DIST_LOSS_KINDS = {"boundary": _ffi.DLOSS_BOUNDARY, "hausdorff dt": _ffi.DLOSS_HAUSDORFF_DT}      # name -> CTL_DLOSS_* kind
DIST_LOSS_FORM = {"boundary": "signed", "hausdorff dt": "squared"}                               # the training form of the label fields a loss reads
DIST_LOSS_NAMES = tuple(DIST_LOSS_KINDS)
LOSS_NAMES = ("cross entropy",) + tuple(LOSS_KINDS) + DIST_LOSS_NAMES
NO_CLASS = 255      # the confident label of a pixel where no class has more than half of the probability
MAX_CLASSES = 16    # channels of a logit / image tensor the loss and statistics kernels take (CTL_ROW_MAXC of csrc/ctl_rows.h); stated once, here


# ---------------------------------------------------------------------------------------------- the rules every loss family shares
def check_names(names, table, noun):
    """ValueError for no name at all, NotImplementedError for a name that is not in `table` (a {name: kind} table or a tuple of names)."""
    if not names:
        raise ValueError(f"{noun}: no names (`kinds` maps at least one name to its weight)")
    for name in names:
        if name not in table:
            raise NotImplementedError(f"{noun} {name!r} (one of {', '.join(table)})")


def check_two_classes(name, c):
    if c < 2:
        raise ValueError(f"{name!r} needs at least 2 classes (it runs over the classes 1 .. C-1)")


def check_constant(t, what):
    if t.requires_grad:
        raise ValueError(f"the {what} is a constant: detach it (no gradient reaches the {what})")


def check_mask(mask, shape):
    """ValueError unless the per-pixel mask (or None) of [B,C,H,W] tensors is [B,1,H,W] or [B,H,W]."""
    b, _, h, w = shape
    if mask is not None and tuple(mask.shape) not in ((b, 1, h, w), (b, h, w)):
        raise ValueError(f"the mask is per pixel: [{b},1,{h},{w}] or [{b},{h},{w}], got {tuple(mask.shape)}")


def mask01(mask, shape, dtype, device):
    """The mask of [B,C,H,W] tensors as [B,1,H,W] zeros and ones, nonzero -> 1; ones without a mask."""
    b, _, h, w = shape
    if mask is None:
        return torch.ones((b, 1, h, w), dtype=dtype, device=device)
    return _nonzero(mask).reshape(b, 1, h, w).to(device=device, dtype=dtype)


def mask_u8(mask):
    """A mask of any dtype as a contiguous uint8 constant (None stays None): what the loss Functions save and the kernels read.  The
    kernels take every nonzero byte as 1, so a contiguous uint8 mask is used as it is."""
    if mask is None or (mask.dtype == torch.uint8 and mask.is_contiguous()):
        return mask
    return _nonzero(mask).to(torch.uint8).contiguous()


def _nonzero(mask):
    return mask.detach() != 0          # nonzero = 1, whatever the mask's dtype


def class_weight_tuple(class_weights, c=None):
    """The class weights (a sequence or a tensor; None stays None) as a tuple of floats, one per class where the class count is known."""
    if class_weights is None:
        return None
    vals = tuple(float(v) for v in (class_weights.flatten().tolist() if hasattr(class_weights, "tolist") else class_weights))
    if c is not None and len(vals) != c:
        raise ValueError(f"each class must have a weight: expected {c} weights, got {len(vals)}")
    return vals


def needs_fields(loss_type):
    """The forms of the label's class fields (ops.class_fields) that a loss name or {name: weight} mapping reads, in its order: empty
    without a distance-map loss."""
    return [DIST_LOSS_FORM[n] for n in (loss_type if isinstance(loss_type, Mapping) else (loss_type,)) if n in DIST_LOSS_FORM]


def parse_loss_type(loss_type, class_weights=None, num_classes=None):
    """[(name, weight)] of a loss name or a {name: weight} mapping, and the class weights as a tuple of floats (or None).  Unknown names and
    'contour_smooth' raise NotImplementedError; class weights of the wrong length, an empty mapping and 'foreground dice', 'boundary' or
    'hausdorff dt' of one class raise ValueError."""
    terms = [(k, float(v)) for k, v in loss_type.items()] if isinstance(loss_type, Mapping) else [(loss_type, 1.0)]
    check_names([n for n, _ in terms], LOSS_NAMES, "segmentation loss")
    class_weights = class_weight_tuple(class_weights, num_classes)
    for n, _ in terms:
        if num_classes is not None and (n == "foreground dice" or n in DIST_LOSS_NAMES):
            check_two_classes(n, num_classes)
    return terms, class_weights


def normalised_weights(class_weights, c):
    """w' = w / sum(w) * C in float64 (custom_loss.py:733-734); None = upstream's uniform 1/C, i.e. ones."""
    if class_weights is None:
        return torch.ones(c, dtype=torch.float64)
    w = torch.tensor(class_weight_tuple(class_weights, c), dtype=torch.float64)
    total = float(w.sum())
    if not (total > 0.0 and total != float("inf")):
        raise ValueError(f"the class weights sum to {total}: a finite, positive sum is needed")
    return w / total * c


def class_fields_host(label, n_class):
    """F[B,C,H,W], float64: the class fields of a label map [B,H,W] as the module docstring defines them, with scipy's exact transform."""
    import numpy as np
    from scipy.ndimage import distance_transform_edt
    y = label.detach().cpu().numpy() if isinstance(label, torch.Tensor) else np.asarray(label)
    f = np.zeros((y.shape[0], int(n_class)) + y.shape[1:], dtype=np.float64)
    for b in range(y.shape[0]):
        for k in range(int(n_class)):
            s = y[b] == k
            if s.any() and not s.all():
                f[b, k] = distance_transform_edt(~s) + distance_transform_edt(s)
    return torch.from_numpy(f)


def signed_from_fields(fields, label):
    """phi[B,C,H,W], float64: F outside the class, -(F - 1) inside, 0 where the field is 0 (an absent or plane-filling class)."""
    f = fields.double()
    inside = label.detach().long().cpu().unsqueeze(1) == torch.arange(f.shape[1]).view(1, -1, 1, 1)
    return torch.where(inside & (f > 0), -(f - 1.0), f)


def confident_label_host(logit, margin=1e-5):
    """(q, near): q uint8 [B,H,W] = the class whose float64 softmax probability exceeds 1/2, NO_CLASS where none does; near bool [B,H,W] =
    the pixels where some |p_k - 1/2| < margin, whose q an fp32 softmax may decide the other way."""
    p = torch.softmax(logit.detach().double().cpu(), 1)
    hit = p > 0.5
    q = torch.where(hit.any(1), hit.double().argmax(1), torch.full((), NO_CLASS, dtype=torch.long)).to(torch.uint8)
    return q, ((p - 0.5).abs() < margin).any(1)


def _dist_one(x, y, name, pred_fields):
    b, c, h, w = x.shape
    div = float(b * (c - 1) * h * w)
    p = torch.softmax(x, 1)
    fg = torch.ones(c, dtype=torch.float64).view(1, c, 1, 1)
    fg[0, 0] = 0.0
    ft = class_fields_host(y, c)
    if name == "boundary":
        phi = signed_from_fields(ft, y)
        loss, g = (fg * p * phi).sum() / div, fg * phi / div
    else:
        t = (y.unsqueeze(1) == torch.arange(c).view(1, c, 1, 1)).double()
        fp = class_fields_host(confident_label_host(x)[0], c) if pred_fields is None else pred_fields.detach().double().cpu()
        d2 = torch.round(ft * ft) + torch.round(fp * fp)
        loss, g = (fg * (p - t) ** 2 * d2).sum() / div, fg * 2.0 * (p - t) * d2 / div
    return loss, p * (g - (p * g).sum(1, keepdim=True))


def _one(x, y, name, class_weights, gamma, pred_fields=None):
    if name in DIST_LOSS_NAMES:
        return _dist_one(x, y, name, pred_fields)
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
    sel = torch.ones(c, dtype=torch.float64)
    if fg:
        sel[0] = 0.0
    div = float(b * (c - 1 if fg else c))
    spt, u = (p * t).sum((2, 3)), p.sum((2, 3)) + t.sum((2, 3)) + SMOOTH
    num = 2.0 * spt + SMOOTH if fg else 2.0 * (spt + SMOOTH)
    g = -(sel.view(1, c, 1, 1) / div) * (2.0 * t / u[:, :, None, None] - (num / (u * u))[:, :, None, None])
    return 1.0 - (sel * num / u).sum() / div, p * (g - (p * g).sum(1, keepdim=True))


def loss_and_grad(logit, label, loss_type="cross entropy", class_weights=None, gamma=2.0, gout=1.0, pred_fields=None):
    """(loss, gout * dloss/dlogit), float64 CPU tensors (0-d and [B,C,H,W]) of a name or a {name: weight} mapping.  `pred_fields`
    ('hausdorff dt' only): the class fields F[B,C,H,W] of the prediction to use instead of those of confident_label_host(logit)."""
    x, y = logit.detach().double().cpu(), label.detach().long().cpu()
    if x.dim() != 4 or y.shape != (x.shape[0], x.shape[2], x.shape[3]):
        raise ValueError("expected logits [B,C,H,W] and a label map [B,H,W]")
    terms, class_weights = parse_loss_type(loss_type, class_weights, x.shape[1])
    loss, grad = torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    for name, weight in terms:
        l, g = _one(x, y, name, class_weights, float(gamma), pred_fields)
        loss, grad = loss + weight * l, grad + weight * g
    return loss, grad * float(gout)


def loss_value(logit, label, loss_type="cross entropy", class_weights=None, gamma=2.0):
    return loss_and_grad(logit, label, loss_type, class_weights, gamma)[0]
