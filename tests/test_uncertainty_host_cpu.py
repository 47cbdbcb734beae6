"""The float64 host statements of uncertainty.py against upstream's recorded outputs (tests/golden/uncertainty_cases.pt, written by
tools/gen_golden_uncertainty.py from the reference's cal_entropy_maps / cal_batch_entropy_maps / CustomBrierLoss), against a plain-loop
ECE written here, and against the properties the definition states.  No GPU."""
import os

import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import uncertainty as U
from cooperative_training_and_latent_space_data_augmentation_amd.metrics import runningMySegmentationScore

GOLDEN = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uncertainty_cases.pt"))
TOL = 1e-12


def _id(case):
    return "x".join(map(str, case["probs"].shape)) + f"-eps{case['eps']}-thr{case['threhold']}-{'max' if case['use_max'] else 'sum'}"


@pytest.mark.parametrize("case", GOLDEN["entropy"], ids=_id)
def test_numpy_path_of_the_entropy_maps_is_upstreams(case):
    p = case["probs"].numpy()
    fn = U.cal_entropy_maps if p.ndim == 3 else U.cal_batch_entropy_maps
    got = fn(p.copy(), eps=case["eps"], threhold=case["threhold"], use_max=case["use_max"])
    want = case["entropy"].numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.max(np.abs(got - want)) <= TOL
    assert (p == case["probs"].numpy()).all()                                  # the input is not written


@pytest.mark.parametrize("case", GOLDEN["entropy"], ids=_id)
def test_host_statement_gives_upstreams_entropy(case):
    """is_prob: H of the statement is upstream's summed form, -conf log2(conf + eps) its use_max form, the threshold applied on top"""
    p = case["probs"].numpy()
    batch = p[None] if p.ndim == 3 else p
    r = U.predictive_stats_host(batch, None, members=1, n_bins=15, eps=case["eps"], is_prob=True)
    ent = -r.conf * np.log2(r.conf + case["eps"]) if case["use_max"] else r.entropy.copy()
    ent[ent < case["threhold"]] = 0.0
    want = case["entropy"].numpy().reshape(ent.shape)
    assert np.max(np.abs(ent - want)) <= TOL
    assert (r.mi == 0).all() and r.stats[:, [0, 1, 4, 5]].sum() == 0 and r.bins.sum() == 0      # one member, no label
    assert np.max(np.abs(r.stats[:, 2] - r.entropy.sum(axis=(1, 2)))) <= TOL


@pytest.mark.parametrize("case", GOLDEN["brier"], ids=lambda c: f"c{c['c']}")
def test_host_statement_gives_upstreams_brier(case):
    """CustomBrierLoss divides the double sum by batch * classes, the statement's mean by the pixel count"""
    x, y, c = case["logit"].numpy(), case["label"].numpy(), case["c"]
    r = U.predictive_stats_host(x, y, members=1)
    assert r.stats[:, 0].sum() == y.size
    upstream_form = r.stats[:, 5].sum() / (x.shape[0] * c)
    assert abs(upstream_form - case["loss"]) <= TOL * max(1.0, abs(case["loss"]))
    cal = U.calibration_from_tables(r.stats, r.bins)
    assert abs(cal["Brier"] * y.size / (x.shape[0] * c) - case["loss"]) <= TOL * max(1.0, abs(case["loss"]))
    logp = torch.log_softmax(case["logit"], dim=1)
    nll = torch.nn.functional.nll_loss(logp, case["label"]).item()
    assert abs(cal["NLL"] - nll) <= TOL * max(1.0, nll)


def random_case(seed, t=1, n=3, c=4, h=16, w=16, bad=True):
    rng = np.random.default_rng(seed)
    x = 3.0 * rng.standard_normal((t * n, c, h, w))
    y = rng.integers(0, c, (n, h, w))
    if bad:
        y[rng.random((n, h, w)) < 0.2] = 255
        y[0, 0, 0] = -1
    return x, y


def plain_loop_ece(conf, correct, n_bins):
    """per-bin boolean masks over the float32 edges the definition names"""
    edges = [np.float64(np.float32(j) / np.float32(n_bins)) for j in range(n_bins + 1)]
    total, ece = conf.size, 0.0
    for j in range(n_bins):
        lo_ok = conf > edges[j] if j > 0 else np.ones_like(conf, dtype=bool)
        hi_ok = conf <= edges[j + 1] if j < n_bins - 1 else np.ones_like(conf, dtype=bool)
        m = lo_ok & hi_ok
        if m.any():
            ece += m.sum() / total * abs(correct[m].mean() - conf[m].mean())
    return ece


@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("n_bins", [1, 10, 15, 64])
def test_ece_against_a_plain_loop(t, n_bins):
    x, y = random_case(100 + t, t=t)
    r = U.predictive_stats_host(x, y, members=t, n_bins=n_bins)
    cal = U.calibration_from_tables(r.stats, r.bins, pixels=y.size)
    valid = (y >= 0) & (y < 4)
    conf, correct = r.conf[valid], (r.pred == y)[valid]
    assert abs(cal["ECE"] - plain_loop_ece(conf, correct, n_bins)) <= TOL
    assert abs(cal["accuracy"] - correct.mean()) <= TOL
    assert r.bins[..., 0].sum() == valid.sum() == r.stats[:, 0].sum() and r.bins[..., 1].sum() == correct.sum() == r.stats[:, 1].sum()
    assert abs(cal["Entropy"] - r.entropy.mean()) <= TOL
    # independent softmax: mean of the members' probabilities
    p = torch.softmax(torch.from_numpy(x), dim=1).numpy().reshape(t, 3, 4, 16, 16).mean(axis=0)
    assert np.max(np.abs(p - r.mean_prob)) <= TOL
    assert abs(cal["NLL"] - (-np.log(np.take_along_axis(p, np.where(valid, y, 0)[:, None], 1)[:, 0][valid]).mean())) <= 1e-11
    if t == 1:
        assert (r.mi == 0).all()
    else:
        assert r.mi.min() > -1e-6 and r.mi.max() > 1e-3                        # Jensen (up to the eps inside the logarithm)
    # the device's fixed-point table gives the same scores
    fixed = np.concatenate([r.bins[..., :2], np.round(r.bins[..., 2:] * U.CONF_SCALE)], axis=-1).astype(np.int64)
    cal_fixed = U.calibration_from_tables(r.stats, fixed, pixels=y.size)
    assert all(abs(cal[k] - cal_fixed[k]) <= 1e-9 for k in cal)


def test_definition_edge_cases():
    # saturated rows: entropy 0, nll finite (160 for the far class), nothing NaN
    x = np.zeros((1, 3, 1, 3))
    x[0, :, 0, 0] = (80.0, -80.0, 0.0)
    x[0, :, 0, 1] = (-80.0, 80.0, 0.0)
    x[0, :, 0, 2] = (0.5, 0.5, 0.5)
    y = np.array([[[1, 1, 7]]])
    r = U.predictive_stats_host(x, y, n_bins=15)
    assert np.isfinite(r.entropy).all() and abs(r.entropy[0, 0, 0]) < 1e-6 and abs(r.entropy[0, 0, 2] - np.log2(3.0)) < 1e-6
    assert abs(r.nll[0, 0, 0] - 160.0) < 1e-9 and abs(r.nll[0, 0, 1]) < 1e-9 and np.isnan(r.nll[0, 0, 2])
    assert r.stats[0, 0] == 2 and r.stats[0, 1] == 1 and list(r.pred[0, 0]) == [0, 1, 0]      # the tie -> the lowest index
    # eps = 0: a zero probability contributes 0
    p = np.array([[[[1.0]], [[0.0]]]])
    assert U.predictive_stats_host(p, None, eps=0.0, is_prob=True).entropy[0, 0, 0] == 0.0
    # uniform logits, 5 classes, 15 bins: conf = 0.2 sits under the float32 edge 3/15
    u = np.full((1, 5, 1, 1), 0.7)
    ru = U.predictive_stats_host(u, np.zeros((1, 1, 1), dtype=np.int64), n_bins=15)
    assert ru.bins[0, :, 0].argmax() == 2 and ru.bins[0, :, 0].sum() == 1
    # all labels out of range: tables zero, maps still there
    rz = U.predictive_stats_host(x, np.full((1, 1, 3), -3))
    assert rz.stats[0, [0, 1, 4, 5]].sum() == 0 and rz.bins.sum() == 0 and np.isfinite(rz.entropy).all()
    cal = U.calibration_from_tables(rz.stats, rz.bins, pixels=3)
    assert np.isnan(cal["ECE"]) and np.isnan(cal["NLL"]) and np.isfinite(cal["Entropy"])
    with pytest.raises(ValueError):
        U.predictive_stats_host(x, y, members=2)
    with pytest.raises(ValueError):
        U.predictive_stats_host(x, y, n_bins=65)


def test_metric_columns_from_numpy_logits():
    """patient-level columns after the per-class ones; today's header and rows are unchanged; chunks concatenate; no logits -> ValueError"""
    x, y = random_case(7, n=6, h=8, w=8, bad=False)
    pred = x.argmax(axis=1)
    names = {0: "BG", 1: "LV", 2: "MYO", 3: "RV"}
    old = runningMySegmentationScore(4, names, metrics_list=("Dice", "VolError"))
    new = runningMySegmentationScore(4, names, metrics_list=("Dice", "ECE", "VolError", "NLL", "Brier", "Entropy"))
    assert new.header == old.header + ["ECE", "NLL", "Brier", "Entropy"]
    row_old = old.update("p0", pred, y)
    row_new = new.update("p0", pred, y, logits=x)
    row_chunked = new.update("p0", pred, y, logits=[x[:4], x[4:]])
    assert row_new[:len(row_old)] == row_old and row_chunked == row_new
    r = U.predictive_stats_host(x, y)
    cal = U.calibration_from_tables(r.stats, r.bins, pixels=y.size)
    assert row_new[len(row_old):] == [cal[k] for k in ("ECE", "NLL", "Brier", "Entropy")]
    summary, _, header = new.get_scores()
    assert header[-4:] == ["ECE", "NLL", "Brier", "Entropy"] and abs(summary["NLL_mean"] - cal["NLL"]) < 1e-15
    assert list(new.save_patient_wise_result_to_csv(None).columns) == new.header
    with pytest.raises(ValueError, match="logits"):
        new.update("p1", pred, y)
    two = runningMySegmentationScore(4, names, metrics_list=("NLL",))
    x2 = np.concatenate([x, x[::-1]])
    assert two.update("p0", pred, y, logits=x2, members=2)[-1] == \
        U.calibration_from_tables(*U.predictive_stats_host(x2, y, members=2)[5:7])["NLL"]
