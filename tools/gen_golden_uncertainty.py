#!/usr/bin/env python3
"""Golden vectors of the uncertainty / calibration statements, produced by the REAL reference on the CPU with float64 inputs:
`cal_entropy_maps` / `cal_batch_entropy_maps` (medseg/common_utils/uncertainty.py:7-54; both use_max forms, thresholds 0 and 0.3) and
`CustomBrierLoss` (medseg/models/custom_loss.py:495-511, use_gpu=False).  Build container only:
    python tools/gen_golden_uncertainty.py  ->  tests/golden/uncertainty_cases.pt
Probabilities are the softmax of 3 * N(0, 1) logits with a few exact zeros and one-hot pixels put in (log2(0 + eps) and the eps = 0
form).  Only tensors and numbers are written."""
import os
import sys
import warnings

sys.path.insert(0, os.environ.get("CTL_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from medseg.common_utils.uncertainty import cal_batch_entropy_maps, cal_entropy_maps  # noqa: E402
from medseg.models.custom_loss import CustomBrierLoss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "uncertainty_cases.pt")
FORMS = [(1e-7, 0.0, False), (1e-7, 0.0, True), (1e-7, 0.3, False), (1e-7, 0.3, True), (1e-3, 0.0, False)]


def probabilities(shape, g):
    """softmax over axis -3 of 3 * N(0, 1); pixel (0, 0) of every image is one-hot, pixel (1, 1) has one exact zero"""
    p = torch.softmax(torch.randn(*shape, generator=g, dtype=torch.float64) * 3.0, dim=-3)
    p[..., :, 0, 0] = 0.0
    p[..., 1, 0, 0] = 1.0
    moved = p[..., 0, 1, 1].clone()
    p[..., 0, 1, 1] = 0.0
    p[..., 1, 1, 1] += moved
    return p


def main():
    warnings.simplefilter("ignore")
    g = torch.Generator().manual_seed(23)
    entropy = []
    for shape in ((4, 7, 9), (3, 5, 6, 5), (2, 2, 3, 4)):
        p = probabilities(shape, g)
        fn = cal_entropy_maps if len(shape) == 3 else cal_batch_entropy_maps
        for eps, thr, use_max in FORMS:
            out = fn(p.numpy().copy(), eps=eps, threhold=thr, use_max=use_max)
            assert out.dtype == np.float64
            entropy.append({"probs": p, "eps": eps, "threhold": thr, "use_max": use_max, "entropy": torch.from_numpy(out.copy())})
    brier = []
    for c in (2, 4, 5):
        x = torch.randn(3, c, 7, 9, generator=g, dtype=torch.float64) * 3.0
        y = torch.randint(0, c, (3, 7, 9), generator=g)
        loss = CustomBrierLoss(n_classes=c, use_gpu=False)(x, y)
        brier.append({"c": c, "logit": x, "label": y, "loss": float(loss)})
    torch.save({"entropy": entropy, "brier": brier}, OUT)
    print(f"wrote {OUT}: {len(entropy)} entropy cases, {len(brier)} Brier cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
