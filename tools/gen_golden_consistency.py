#!/usr/bin/env python3
"""Golden vectors of the consistency losses, produced by the REAL reference (medseg/models/custom_loss.py) on the CPU.  Build container only:
    python tools/gen_golden_consistency.py  ->  tests/golden/consistency_cases.pt
Shapes follow loss_cases.pt: (3, C, 7, 9) for C in {2, 4, 5}, distinct class weights.  Recorded, each with the loss and d loss / d output:
  'kl', 'mse'            calc_segmentation_consistency(scales=[0]), float64, without and with a [3,1,7,9] 0/1 mask, is_gt False / True (one-hot)
  'ce', 'weighted ce'    the same entry, no mask (upstream raises with one), both is_gt
  'Dice'                 SoftDiceLoss(C, use_gpu=False)(x, r, mask=None | m.view(3,1,-1), is_gt=...) directly, float64 (the entry above raises)
  'contour'              contour_loss(input=q[:, [k]], target=p[:, [k]], use_gpu=False, ignore_background=False, one_hot_target=False, mask=...)
                         per class k >= 1, averaged as :959-965 does, in float32 (the only dtype its filters accept).  q and p are
                         probabilities that are multiples of 2^-4 with rows summing to 1, so every Sobel sum and square is exact in
                         float32; the recorded gradient is d loss / d q.
Only tensors and numbers are written."""
import contextlib
import io
import os
import sys
import warnings

sys.path.insert(0, os.environ.get("CTL_REFERENCE", "/root/reference"))

import torch  # noqa: E402

from medseg.models.custom_loss import SoftDiceLoss, calc_segmentation_consistency, contour_loss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "consistency_cases.pt")


def sixteenths(c, g):
    """[3,c,7,9] float32 probabilities: positive multiples of 1/16 that sum to 1 over c."""
    extra = torch.zeros(3, c, 7, 9)
    idx = torch.randint(0, c, (16 - c, 3, 7, 9), generator=g)
    for i in range(16 - c):
        extra.scatter_add_(1, idx[i].unsqueeze(1), torch.ones(3, 1, 7, 9))
    return (extra + 1.0) / 16.0


def main():
    warnings.simplefilter("ignore")
    g = torch.Generator().manual_seed(23)
    cases = []

    def record(name, c, fn, x, **kw):
        xr = x.clone().requires_grad_(True)
        with contextlib.redirect_stdout(io.StringIO()):           # (upstream prints every term)
            loss = fn(xr)
        assert loss.dtype == x.dtype, (name, loss.dtype)
        grad, = torch.autograd.grad(loss, [xr])
        cases.append(dict(name=name, c=c, output=x, loss=float(loss), grad=grad, **kw))

    for c in (2, 4, 5):
        x = torch.randn(3, c, 7, 9, generator=g, dtype=torch.float64) * 3.0
        r = torch.randn(3, c, 7, 9, generator=g, dtype=torch.float64) * 3.0
        y = torch.randint(0, c, (3, 7, 9), generator=g)
        onehot = torch.nn.functional.one_hot(y, c).permute(0, 3, 1, 2).double().contiguous()
        m = (torch.rand(3, 1, 7, 9, generator=g) < 0.6).double()
        w = [0.5 + 0.75 * k + 0.1 * (k % 2) for k in range(c)]
        wt = torch.tensor(w, dtype=torch.float64)
        for is_gt, ref in ((False, r), (True, onehot)):
            for name in ("kl", "mse", "ce", "weighted ce"):
                for mask in ((None, m) if name in ("kl", "mse") else (None,)):
                    record(name, c, lambda xr: calc_segmentation_consistency(
                        xr, ref, divergence_types=[name], divergence_weights=[1.0], class_weights=w if name == "weighted ce" else None,
                        scales=[0], mask=None if mask is None else mask.clone(), is_gt=is_gt),
                        x, reference=ref, mask=mask, is_gt=is_gt, class_weights=wt, dtype="float64")
            for mask in (None, m):
                record("Dice", c, lambda xr: SoftDiceLoss(n_classes=c, use_gpu=False)(
                    xr, ref, mask=None if mask is None else mask.view(3, 1, -1), is_gt=is_gt),
                    x, reference=ref, mask=mask, is_gt=is_gt, class_weights=wt, dtype="float64")
        q, p = sixteenths(c, g), sixteenths(c, g)
        for mask in (None, m.float()):
            def contour(qr):
                loss = 0.0
                for k in range(1, c):
                    loss = loss + contour_loss(input=qr[:, [k]], target=p[:, [k]], use_gpu=False, ignore_background=False,
                                               one_hot_target=False, mask=mask)
                return loss / (c - 1)
            record("contour", c, contour, q, reference=p, mask=mask, is_gt=True, class_weights=wt, dtype="float32")
    torch.save({"cases": cases}, OUT)
    print(f"wrote {OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
