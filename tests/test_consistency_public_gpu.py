"""The public consistency functions on the device: calc_segmentation_consistency, kl_divergence and the two wrappers against the ops calls
they are made of (bit for bit), the recorded upstream cases moved to the device (within the bounds tests/test_consistency_gpu.py derives
from the number formats), and the solver's consistency_training on the smallest configuration of the solver tests."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as O  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import autograd, consistency as K, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel, basic_loss_fn  # noqa: E402
from test_consistency_gpu import U, kind_bounds  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consistency_cases.pt")
CH_MSE = {"loss_name": "mse", "mask_type": "channel", "max_threshold": 0.5, "random_threshold": False, "if_soft": False}
SP_CE = {"loss_name": "ce", "mask_type": "spatial", "max_threshold": 0.5, "random_threshold": False, "if_soft": False}
NAMES = ["kl", "ce", "weighted ce", "mse", "Dice", "contour"]
WEIGHTS = [1.0, 0.5, 0.3, 2.0, 0.7, 1.5]
CW = [0.5, 1.0, 2.5, 1.5]


def dev(x):
    x = x.to(DEV)
    return x.contiguous(memory_format=torch.channels_last) if x.dim() == 4 else x.contiguous()


def pair(b=2, c=4, h=17, w=31, seed=1):
    g = torch.Generator().manual_seed(seed)
    return dev(torch.randn(b, c, h, w, generator=g) * 3.0), dev(torch.randn(b, c, h, w, generator=g) * 3.0)


def test_public_function_is_the_ops_calls():
    x, r = pair()
    mask = (torch.rand(2, 1, 17, 31, generator=torch.Generator().manual_seed(2)) < 0.6).float().to(DEV)
    kinds = dict(zip(NAMES, WEIGHTS))
    one = torch.ones((), device=DEV)
    # scales = [0]: one fused call, with and without a mask
    for m in (None, mask):
        xr = x.clone().requires_grad_(True)
        loss = K.calc_segmentation_consistency(xr, r, NAMES, WEIGHTS, CW, [0], m)
        loss.backward()
        want, _, ws = ops.consistency_fwd(x, r, kinds, CW, m)
        assert loss.dtype == torch.float32 and torch.equal(loss.detach(), want)
        assert torch.equal(xr.grad, ops.consistency_bwd(x, r, kinds, one, ws, CW, m))
    # scales = [0, 1]: (L_0 + 2 L_1) / 2 with L_1 on the pooled pair, the gradient chained through the pooling
    xr = x.clone().requires_grad_(True)
    loss = K.calc_segmentation_consistency(xr, r, NAMES, WEIGHTS, CW, [0, 1])
    loss.backward()
    x1, r1 = ops.avgpool_fwd(x, 1), ops.avgpool_fwd(r, 1)
    l0, _, ws0 = ops.consistency_fwd(x, r, kinds, CW)
    l1, _, ws1 = ops.consistency_fwd(x1, r1, kinds, CW)
    assert torch.equal(loss.detach(), (l0 * 1.0 + l1 * 2.0) / 2.0)
    g0 = ops.consistency_bwd(x, r, kinds, one * 0.5, ws0, CW)
    g1 = ops.avgpool_bwd(ops.consistency_bwd(x1, r1, kinds, one * 0.5 * 2.0, ws1, CW), 1, (17, 31))
    assert torch.equal(xr.grad, g0 + g1) or torch.equal(xr.grad, g1 + g0)
    ref_loss, ref_grad = K.consistency_and_grad(x.cpu(), r.cpu(), NAMES, WEIGHTS, CW, [0, 1])
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    assert float((xr.grad.cpu().double() - ref_grad).abs().max()) <= 1e-5 * float(ref_grad.abs().max())
    # autograd.avg_pool alone
    xr = x.clone().requires_grad_(True)
    y = autograd.avg_pool(xr, 2)
    assert torch.equal(y.detach(), ops.avgpool_fwd(x, 2))
    gy = torch.randn_like(y)
    y.backward(gy)
    assert torch.equal(xr.grad, ops.avgpool_bwd(dev(gy), 2, (17, 31)))


def test_wrappers_are_the_special_cases():
    x, r = pair(seed=4)
    mask = (torch.rand(2, 17, 31, generator=torch.Generator().manual_seed(5)) < 0.5).to(DEV)
    onehot = dev(torch.nn.functional.one_hot(torch.randint(0, 4, (2, 17, 31), generator=torch.Generator().manual_seed(6)), 4).permute(0, 3, 1, 2).float())
    assert torch.equal(K.kl_divergence(r, x), ops.consistency_fwd(x, r, {"kl": 1.0})[0])
    assert torch.equal(K.kl_divergence(r, x, mask=mask), ops.consistency_fwd(x, r, {"kl": 1.0}, mask=mask)[0])
    assert torch.equal(K.kl_divergence(onehot, x, is_gt=True), ops.consistency_fwd(x, onehot, {"kl": 1.0}, is_gt=True)[0])
    assert torch.equal(K.calc_segmentation_kl_consistency(x, r), ops.consistency_fwd(x, r, {"kl": 1.0})[0])
    assert torch.equal(K.calc_segmentation_mse_consistency(x, r), ops.consistency_fwd(x, r, {"mse": 1.0})[0])
    assert torch.equal(K.calc_segmentation_consistency(x, r), ops.consistency_fwd(x, r, {"kl": 1.0, "contour": 0.5})[0])      # the defaults
    with pytest.raises(ValueError, match="constant"):
        K.calc_segmentation_consistency(x, r.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="mask"):
        K.calc_segmentation_consistency(x, r, scales=[0, 1], mask=mask)
    # the rules that only device tensors reach: every layer that takes the argument states them in the same words
    x8, r8 = pair(2, 4, 8, 8, seed=7)
    one, ws = torch.ones((), device=DEV), torch.zeros(64, dtype=torch.float64, device=DEV)
    kl = {"kl": 1.0}
    for bad in (torch.ones(2, 2, 8, 8, device=DEV), torch.ones(1, 1, 8, 8, device=DEV), torch.ones(2, 8, 7, device=DEV)):
        for fn in (lambda: K.calc_segmentation_consistency(x8, r8, mask=bad), lambda: autograd.consistency_loss(x8, r8, kl, mask=bad),
                   lambda: ops.consistency_fwd(x8, r8, kl, mask=bad), lambda: ops.consistency_bwd(x8, r8, kl, one, ws, mask=bad)):
            with pytest.raises(ValueError, match=r"the mask is per pixel: \[2,1,8,8\] or \[2,8,8\]"):
                fn()
    x1, r1 = pair(2, 1, 8, 8, seed=8)
    y1, contour = torch.zeros(2, 8, 8, dtype=torch.long, device=DEV), {"contour": 1.0}
    for name, fns in (("contour", (lambda: K.calc_segmentation_consistency(x1, r1, ["contour"], [1.0]), lambda: autograd.consistency_loss(x1, r1, contour),
                                   lambda: ops.consistency_fwd(x1, r1, contour), lambda: ops.consistency_bwd(x1, r1, contour, one, ws))),
                      ("boundary", (lambda: basic_loss_fn(x1, y1, "boundary"), lambda: autograd.segmentation_loss(x1, y1, "boundary"),
                                    lambda: ops.dist_loss_fwd(x1, y1, "boundary", x1), lambda: ops.dist_loss_bwd(x1, y1, "boundary", one, x1))),
                      ("hausdorff dt", (lambda: autograd.segmentation_loss(x1, y1, "hausdorff dt"), lambda: ops.dist_loss_fwd(x1, y1, "hausdorff dt", x1, x1)))):
        for fn in fns:
            with pytest.raises(ValueError, match=f"'{name}' needs at least 2 classes"):
                fn()
    xs, rs = pair(2, 1, 2, 2, seed=9)
    for fn in (lambda: K.calc_segmentation_consistency(xs, rs, ["mse"], [1.0], scales=[2]), lambda: autograd.avg_pool(xs, 2), lambda: ops.avgpool_fwd(xs, 2)):
        with pytest.raises(ValueError, match="a 2x2 plane is smaller than the 4x4 window of scale 2"):
            fn()


def test_recorded_upstream_cases_on_the_device():
    """The recorded float64 cases (rounded to fp32 on the way in) and the float32 contour cases (x = log q, is_gt), within the bounds
    kind_bounds derives for the fp32 inputs plus one rounding of the result; the reference is the host statement on the same fp32 inputs,
    which tests/test_consistency_host_cpu.py holds against upstream at 1e-12."""
    cases = torch.load(GOLDEN, weights_only=True)["cases"]
    worst = {}
    for q in cases:
        name, c = q["name"], q["c"]
        x = (torch.log(q["output"].double()) if name == "contour" else q["output"]).float().contiguous(memory_format=torch.channels_last)
        r = q["reference"].float().contiguous(memory_format=torch.channels_last)
        cw = q["class_weights"].tolist() if name == "weighted ce" else None
        mask = q["mask"]
        xd = x.to(DEV).requires_grad_(True)
        loss = K.calc_segmentation_consistency(xd, r.to(DEV), [name], [1.0], cw, [0], None if mask is None else mask.to(DEV), q["is_gt"])
        loss.backward()
        ref_loss, ref_grad = K.consistency_and_grad(x, r, [name], [1.0], cw, [0], mask, q["is_gt"])
        lb, gb = kind_bounds(name, x, r, None if mask is None else mask.reshape(3, 7, 9), q["is_gt"], cw)
        lb = 1.001 * lb + U * abs(float(ref_loss)) + 1e-12
        gb = 1.001 * gb + U * ref_grad.abs() + 1e-12 * float(ref_grad.abs().max()) + 1e-30
        lf = abs(float(loss) - float(ref_loss)) / lb
        gf = float(((xd.grad.cpu().double() - ref_grad).abs() / gb).max())
        worst[name] = (max(worst.get(name, (0, 0))[0], lf), max(worst.get(name, (0, 0))[1], gf))
        assert lf <= 1.0 and gf <= 1.0, (name, c, q["is_gt"], mask is not None, lf, gf)
        if q["dtype"] == "float64":      # and upstream's own number, at the fp32 rounding of the inputs (a loose sanity figure, not the bound)
            assert abs(float(loss) - q["loss"]) <= 2e-5 * max(1.0, abs(q["loss"])), (name, c, float(loss), q["loss"])
    print("recorded cases on the device (loss error / bound, gradient error / bound): " + "; ".join(f"{k}: {v[0]:.3f} / {v[1]:.3f}" for k, v in worst.items()))


def _solver(golden_sd):
    s = AdvancedTripletReconSegmentationModel(use_gpu=True)
    for k, m in s.model.items():
        m.load_state_dict(golden_sd[k])
    return s


@pytest.fixture(scope="module")
def batch():
    return tuple(dev(t) for t in O.synthetic_batch(2, 64, 64, seed=5))      # the smallest batch and image size of the engine tests


@pytest.mark.parametrize("target", ["stn", "ftn"])
def test_consistency_training(golden_sd, batch, target):
    clean, label, noisy = batch
    types, weights = ["kl", "contour", "mse"], [1.0, 0.5, 0.25]
    s = _solver(golden_sd)
    s.train()
    s.zero_grad()
    loss = s.consistency_training(clean, noisy, target=target, divergence_types=types, divergence_weights=weights)
    assert loss.dim() == 0 and loss.requires_grad and bool(torch.isfinite(loss))
    # the hand composition, bit for bit
    with torch.no_grad():
        y_ref = s.fast_predict(clean, disable_track_bn_stats=True)[1]
        if target == "stn":
            y_ref = s.recon_shape(y_ref, is_label_map=False, disable_track_bn_stats=True)
    y = s.fast_predict(noisy, disable_track_bn_stats=True)[1]
    hand = K.calc_segmentation_consistency(y, y_ref.detach(), types, weights)
    assert torch.equal(hand.detach(), loss.detach())
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: m._flat.grad.detach().clone() for k, m in s.model.items()}
    for k in ("image_encoder", "segmentation_decoder"):
        assert bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0.0, k
    for k in ("shape_encoder", "shape_decoder", "image_decoder"):
        assert float(grads[k].abs().max()) == 0.0, k
    # a second identical call repeats the bits (BatchNorm statistics are not tracked, nothing was stepped)
    again = s.consistency_training(clean, noisy, target=target, divergence_types=types, divergence_weights=weights)
    assert torch.equal(again.detach(), loss.detach())
    with pytest.raises(ValueError, match="target"):
        s.consistency_training(clean, noisy, target="teacher")


def test_consistency_training_leaks_nothing_into_the_fused_step(golden_sd, batch):
    clean, label, noisy = batch

    def steps(with_call):
        s = _solver(golden_sd)
        out = [torch.stack([v.detach().float() for v in s.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)]).cpu()]
        if with_call:
            s.consistency_training(clean, noisy, target="stn").detach()      # no backward, no optimizer step: the networks stay as they are
        out.append(torch.stack([v.detach().float() for v in s.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)]).cpu())
        return out

    a, b = steps(True), steps(False)
    assert a[0].numel() == 8 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
