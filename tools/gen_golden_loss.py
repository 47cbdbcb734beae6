#!/usr/bin/env python3
"""Golden vectors of the supervised segmentation losses, produced by the REAL reference `basic_loss_fn`
(medseg/models/custom_loss.py:8-40) on the CPU with float64 inputs (use_gpu=False).  Build container only:
    python tools/gen_golden_loss.py  ->  tests/golden/loss_cases.pt
For each of the five names beside 'cross entropy' and C in {2, 4, 5} at 3 x C x 7 x 9: logits, label map, class weights, the loss and
its gradient.  The label map has one class absent from sample 0 and sample 1 made of a single class; the class weights are non-uniform.
Only tensors and numbers are written."""
import os
import sys
import warnings

sys.path.insert(0, os.environ.get("CTL_REFERENCE", "/root/reference"))

import torch  # noqa: E402

from medseg.models.custom_loss import basic_loss_fn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "loss_cases.pt")
NAMES = ["weighted cross entropy", "dice", "weighted dice", "foreground dice", "focal"]


def label_map(c, g):
    y = torch.randint(0, c, (3, 7, 9), generator=g)
    absent = c - 1
    y[0][y[0] == absent] = 0                  # sample 0: one class absent
    y[1] = 1                                  # sample 1: a single class
    for k in range(c):                        # sample 2: every class present
        y[2, k % 7, k] = k
    return y


def main():
    warnings.simplefilter("ignore")           # (FocalLoss calls log_softmax without a dim)
    g = torch.Generator().manual_seed(11)
    cases = []
    for c in (2, 4, 5):
        x = torch.randn(3, c, 7, 9, generator=g, dtype=torch.float64) * 3.0
        y = label_map(c, g)
        w = [0.5 + 0.75 * k + 0.1 * (k % 2) for k in range(c)]
        wt, grads = torch.tensor(w, dtype=torch.float64), []
        for name in NAMES:
            xr = x.clone().requires_grad_(True)
            loss = basic_loss_fn(xr, y, loss_type=name, class_weights=w, use_gpu=False)
            assert loss.dtype == torch.float64, (name, loss.dtype)
            grad, = torch.autograd.grad(loss, [xr])
            grad = next((q for q in grads if torch.equal(q, grad)), grad)      # equal bits ('weighted dice' == 'dice') are stored once
            grads.append(grad)
            # the cases of one C share the input tensors (torch.save writes a shared tensor once)
            cases.append({"name": name, "c": c, "logit": x, "label": y, "class_weights": wt, "loss": float(loss), "grad": grad})
    torch.save({"cases": cases}, OUT)
    print(f"wrote {OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
