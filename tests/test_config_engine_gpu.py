"""Networks and the solver at configurations off the shipped one (image_ch 1, 4 classes, reduce_factor 4): other class counts, 4 image
channels, reduce_factor 8 (widths 8 ... 64: layers with c % 16 != 0 on the fp32 pipe, ungrouped fp32 weight gradients, no fused BatchNorm-
backward prologue there) and reduce_factor 2 (widths 32 ... 256: a full prologue coefficient table).  The bodies, tolerances and inputs
are those of tests/test_engine_gpu.py and tests/test_bf16_engine_gpu.py, with the channel counts of the configuration; the weights are
init.reference_init_state_dicts(*cfg) under torch.manual_seed(0).  Which configurations exist at all: tests/test_config_contract_cpu.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as O  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, init, model_util, nets  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel  # noqa: E402
from test_engine_gpu import (NET_INPUT, PLAN_SWITCHES, _grouped_pass_equals_consecutive_passes, _network_eval_mode_vs_oracle,  # noqa: E402
                             _network_forward_backward_vs_oracle, close, dev)
import test_bf16_engine_gpu as B16  # noqa: E402

FP32_CFGS = [(1, 8, 4), (1, 12, 4), (1, 16, 4), (4, 4, 4), (1, 4, 8), (1, 8, 8), (1, 4, 2)]
BF16_CFGS = [(1, 8, 4), (1, 16, 4), (4, 4, 4), (1, 4, 2)]
WIDTH_CFGS = [(1, 4, 8), (1, 4, 2)]
cid = lambda cfg: "-".join(map(str, cfg))


@functools.lru_cache(maxsize=None)
def weights(cfg):
    torch.manual_seed(0)
    return init.reference_init_state_dicts(*cfg)


# ------------------------------------------------------------------------------------------------ fp32 networks
@pytest.mark.parametrize("name", list(NET_INPUT))
@pytest.mark.parametrize("cfg,mode,switches", [(c, "A", "default") for c in FP32_CFGS] + [((1, 4, 8), "B", "default")]
                         + [(c, "A", s) for c in WIDTH_CFGS for s in ("all_folded", "stand_alone_passes")],
                         ids=lambda v: cid(v) if isinstance(v, tuple) else v)
def test_network_forward_backward_vs_oracle_at_config(name, cfg, mode, switches):
    """tests/test_engine_gpu.py::test_network_forward_backward_vs_oracle, unchanged: outputs 1e-4 abs, dx and parameter gradients
    5e-4 of the tensor's max, buffers 1e-5, dead biases as is_dead_bias"""
    old = {k: getattr(nets, k) for k in PLAN_SWITCHES[switches]}
    for k, v in PLAN_SWITCHES[switches].items():
        setattr(nets, k, v)
    try:
        _network_forward_backward_vs_oracle(name, mode, weights(cfg), cfg)
    finally:
        for k, v in old.items():
            setattr(nets, k, v)


@pytest.mark.parametrize("name", list(NET_INPUT))
@pytest.mark.parametrize("cfg", FP32_CFGS, ids=cid)
def test_network_eval_mode_vs_oracle_at_config(name, cfg):
    """mode C after two training passes (tests/test_engine_gpu.py::test_network_eval_mode_vs_oracle)"""
    _network_eval_mode_vs_oracle(name, weights(cfg), cfg)


def widest_prologue(name, cfg):
    """channels of the widest BatchNorm a consumer conv applies while staging: the encoders' 512 // reduce_factor, the decoders' 256 // reduce_factor"""
    return (512 if name.endswith("encoder") else 256) // cfg[2]


@pytest.mark.parametrize("mode", ["A", "B"])
@pytest.mark.parametrize("name,n", [("shape_encoder", 3), ("shape_decoder", 2), ("image_encoder", 4), ("segmentation_decoder", 5)])
@pytest.mark.parametrize("cfg", WIDTH_CFGS, ids=cid)
def test_grouped_pass_equals_consecutive_passes_at_config(cfg, name, n, mode):
    """Two BatchNorm groups.  At reduce_factor 2 the encoders' latent layers need 2 x 256 prologue coefficients in one launch, twice
    what the conv kernels stage (CTL_PRO_MAX): such a pass is refused as a whole before its first launch, by name; everything else is
    tests/test_engine_gpu.py::test_grouped_pass_equals_consecutive_passes."""
    if 2 * widest_prologue(name, cfg) > nets.PRO_MAX:
        net = nets.build_networks(*cfg, device="cuda", state_dicts={name: weights(cfg)[name]})[name]
        c, h, w = (cfg[0] if name == "image_encoder" else cfg[1]), 48, 64
        x = dev(torch.rand(2 * n, c, h, w))
        launches = int(_ffi.lib.ctl_launch_count())
        with pytest.raises(_ffi.CtlError, match=f"groups \\* cin = {2 * widest_prologue(name, cfg)}"):
            net.run_forward(x, "A", groups=2)
        assert int(_ffi.lib.ctl_launch_count()) == launches, "a refused pass launched something"
        net.run_forward(x, "A", groups=1)                       # the same batch as one group is served
        return
    _grouped_pass_equals_consecutive_passes(name, n, mode, weights(cfg), cfg)


# ------------------------------------------------------------------------------------------------ bf16 networks, forward
@pytest.mark.parametrize("mode", ["A", "C"])
@pytest.mark.parametrize("name", list(B16.NET_INPUT))
@pytest.mark.parametrize("cfg", BF16_CFGS, ids=cid)
def test_bf16_network_forward_vs_rounding_point_oracle_at_config(cfg, name, mode):
    """tests/test_bf16_engine_gpu.py::test_bf16_network_forward_vs_rounding_point_oracle: 128 x 128 / 8 x 8 inputs, 2e-2 max, 3e-3 mean of
    max|ref|, running statistics 5e-3"""
    sd = weights(cfg)
    onet = O.build_networks(*cfg, init=False)[name]
    onet.load_state_dict(sd[name])
    hnet = nets.build_networks(*cfg, device="cuda", state_dicts={name: sd[name]}, dtype="bf16")[name]
    _, h, w = B16.NET_INPUT[name]
    c = {"image_encoder": cfg[0], "shape_encoder": cfg[1]}.get(name, 512 // cfg[2])
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(4, c, h, w, generator=g)) if "decoder" in name else torch.rand(4, c, h, w, generator=g)
    with torch.no_grad(), O.bf16_rounding_points():
        if mode == "C":
            for _ in range(2):
                onet(x * 1.5)
                hnet(dev(x * 1.5))
            onet.eval()
            hnet.eval()
        yo, yh = onet(x), hnet(dev(x))
    errs, means = [], []
    for a, b in zip(yh if isinstance(yh, tuple) else (yh,), yo if isinstance(yo, tuple) else (yo,)):
        assert a.dtype == torch.float32
        errs.append(B16.rel_err(a, b))
        means.append(float((a.cpu().double() - b.double()).abs().mean() / b.double().abs().max()))
    hb = dict(hnet.named_buffers())
    berr = max(float((hb[n].cpu().double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-6))
               for n, b in onet.named_buffers() if b.dtype.is_floating_point)
    print(f"bf16 {cid(cfg)} {name} mode {mode}: output max err {max(errs):.2e} mean err {max(means):.2e} (of max|ref|), running-statistics rel err {berr:.2e}")
    assert max(errs) <= 2e-2 and max(means) <= 3e-3, (name, mode, errs, means)
    assert berr <= 5e-3, (name, mode, berr)


# ------------------------------------------------------------------------------------------------ the solver at 8 classes
CLASSES = 8
BATCH_SEED = 2          # oracle alone, on the CPU: 99.99 % (n_iter 1) and 100 % (n_iter 2) of the pixels have a top-2 logit margin > 2e-4


def _pair8():
    sd = weights((1, CLASSES, 4))
    s = AdvancedTripletReconSegmentationModel(num_classes=CLASSES, use_gpu=True)
    for k, m in s.model.items():
        m.load_state_dict(sd[k])
    return s, O.OracleSolver(num_classes=CLASSES, state_dicts=sd), O.synthetic_batch(4, 64, 64, num_classes=CLASSES, seed=BATCH_SEED)


def test_solver_standard_training_and_predict_at_8_classes():
    s, o, (clean, label, noisy) = _pair8()
    got = s.standard_training(dev(clean), dev(label), dev(noisy))
    ref = o.standard_training(clean, label, noisy)
    for g, r in zip(got, ref):
        assert abs(float(g) - float(r)) < 1e-4, ([float(v) for v in got], [float(v) for v in ref])
    close(s.z_i, o.z_i, what="z_i")
    close(s.z_s, o.z_s, what="z_s")
    for n_iter in (1, 2):                                       # the FTN alone, and refined by one STN pass
        logits = o.predict(noisy, n_iter=n_iter)
        top2 = logits.topk(2, dim=1)[0]
        safe = (top2[:, 0] - top2[:, 1]) > 2e-4
        assert float(safe.float().mean()) >= 0.99
        pred = s.predict(dev(noisy), n_iter=n_iter)
        assert pred.shape[1] == CLASSES
        assert torch.equal(pred.argmax(1).cpu()[safe], logits.argmax(1)[safe]), f"label maps differ away from ties (n_iter {n_iter})"


def test_solver_evaluate_with_device_targets_matches_host_path_at_8_classes():
    (a, _, (clean, label, noisy)), (b, _, _) = _pair8(), _pair8()
    a.evaluate(dev(noisy), label.numpy(), n_iter=2)
    b.evaluate(dev(noisy), dev(label), n_iter=2)
    sa, ia = a.running_metric.get_scores()
    sb, ib = b.running_metric.get_scores()
    assert len(ia) == CLASSES
    assert sa == sb and all((ia[k] == ib[k]) or (np.isnan(ia[k]) and np.isnan(ib[k])) for k in ia)
    cm = np.asarray(a.running_metric.confusion_matrix)
    assert cm.shape == (CLASSES, CLASSES) and int(cm.sum()) == label.numel()


@pytest.mark.parametrize("loss_type", ["ce", "mse"])
def test_saliency_gradient_at_8_classes(loss_type):
    """dL/dz through the frozen segmentation decoder (model_util._saliency_grad) against autograd on the oracle, at the dx tolerance of
    the network tests"""
    s, o, (clean, label, noisy) = _pair8()
    z = torch.relu(torch.randn(4, 128, 4, 4, generator=torch.Generator().manual_seed(5)))
    s.train()
    _, got = model_util._saliency_grad(dev(z), s.model["segmentation_decoder"], dev(label), CLASSES, loss_type)
    ref = O.saliency_grad(z, o.model["segmentation_decoder"], label, CLASSES, loss_type)
    close(got, ref, atol=1e-6, rel=5e-4, what=f"saliency gradient ({loss_type})")
