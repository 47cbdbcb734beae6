"""The host statements of the distance-map losses (losses.py): class fields against the literal lines of Kervadec's one_hot2dist, the zero
rule for absent and plane-filling classes, value and closed-form gradient of 'boundary' and 'hausdorff dt' against torch.autograd on the
float64 formula, the mapping form and the name rules."""
import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt as edt

from cooperative_training_and_latent_space_data_augmentation_amd import losses


def blobs(b, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(b, c, max(1, h // 4 + 1), max(1, w // 4 + 1), generator=g)
    return torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False).argmax(1)


def kervadec(seg, k):
    """one_hot2dist of the boundary-loss code, class k of one slice, for a class that is present"""
    pos = seg == k
    neg = ~pos
    return edt(neg) * neg - (edt(pos) - 1) * pos


@pytest.mark.parametrize("h, w, c", [(9, 13, 3), (16, 16, 4), (5, 31, 2)])
def test_fields_are_kervadecs_lines(h, w, c):
    y = blobs(3, h, w, c, 5)
    f = losses.class_fields_host(y, c)
    phi = losses.signed_from_fields(f, y)
    checked = 0
    for b in range(y.shape[0]):
        for k in range(c):
            s = (y[b] == k).numpy()
            if not s.any() or s.all():
                continue
            checked += 1
            np.testing.assert_array_equal(phi[b, k].numpy(), kervadec(y[b].numpy(), k))
            np.testing.assert_array_equal(f[b, k].numpy(), edt(~s) + edt(s))
            d2 = f[b, k].numpy() ** 2
            assert np.abs(d2 - np.round(d2)).max() < 1e-9                      # a squared distance between pixel centres is an integer
            assert (f[b, k].numpy() >= 1.0).all()
    assert checked >= 4


def test_zero_rule_for_absent_and_full_classes_and_foreign_labels():
    y = torch.zeros(2, 6, 7, dtype=torch.long)
    y[1, 2:4, 3:5] = 2
    y[1, 0, 0] = 255                                                           # no class: belongs to no S
    y[1, 5, 6] = -1
    f = losses.class_fields_host(y, 4)
    assert (f[0] == 0).all()                                                   # class 0 fills the plane, 1..3 are absent
    assert (f[1, 1] == 0).all() and (f[1, 3] == 0).all()
    assert (f[1, 0] > 0).all() and (f[1, 2] > 0).all()
    assert f[1, 0, 0, 0] == 1.0 and f[1, 2, 0, 0] == np.sqrt(13.0)           # the foreign pixel is outside class 0 and outside class 2
    phi = losses.signed_from_fields(f, y)
    assert (phi[0] == 0).all() and (phi[1, 1] == 0).all()
    assert phi[1, 2, 2, 3] == 0.0 and phi[1, 2, 0, 3] == 2.0 and phi[1, 0, 2, 3] == 1.0
    y8 = y.clamp(0, 255).to(torch.uint8)
    y8[1, 5, 6] = 255
    assert torch.equal(losses.class_fields_host(y8, 4), f)


def test_confident_label_host():
    x = torch.tensor([[4.0, 0.0, 0.0], [0.0, 0.0, -12.0], [1.0, 1.0, 1.0], [0.0, 1.0, 3.0]]).t().reshape(1, 3, 2, 2)
    q, near = losses.confident_label_host(x)
    assert q.dtype == torch.uint8 and q.flatten().tolist() == [0, 255, 255, 2]
    assert near.flatten().tolist() == [False, True, False, False]              # two equal top logits: p = 1/2 - 1.5e-6


def formula(x, y, name, ft, fp):
    b, c, h, w = x.shape
    p = torch.softmax(x, 1)
    div = b * (c - 1) * h * w
    if name == "boundary":
        return (p[:, 1:] * losses.signed_from_fields(ft, y)[:, 1:]).sum() / div
    t = (y.unsqueeze(1) == torch.arange(c).view(1, c, 1, 1)).double()
    return (((p - t) ** 2) * (ft ** 2 + fp ** 2))[:, 1:].sum() / div


@pytest.mark.parametrize("name", ["boundary", "hausdorff dt"])
@pytest.mark.parametrize("b, c, h, w", [(2, 4, 9, 11), (1, 2, 5, 5), (3, 5, 8, 6)])
def test_value_and_gradient_against_autograd(name, b, c, h, w):
    g = torch.Generator().manual_seed(b * 100 + c)
    x = (3.0 * torch.randn(b, c, h, w, generator=g, dtype=torch.float64)).requires_grad_()
    y = blobs(b, h, w, c, 7)
    y[0, 0, 0] = 255
    ft = losses.class_fields_host(y, c)
    fp = losses.class_fields_host(losses.confident_label_host(x)[0], c)       # a constant of the gradient
    want = formula(x, y, name, ft, fp)
    want.backward()
    want = want.detach()
    loss, grad = losses.loss_and_grad(x, y, name, gout=0.75)
    assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    scale = max(1.0, float(x.grad.abs().max()))
    assert float((grad - 0.75 * x.grad).abs().max()) <= 1e-12 * scale
    # handing the prediction's fields in is the same statement
    loss2, grad2 = losses.loss_and_grad(x, y, name, gout=0.75, pred_fields=fp)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_boundary_is_negative_for_the_true_segmentation():
    y = blobs(2, 12, 12, 3, 3)
    x = 20.0 * torch.nn.functional.one_hot(y, 3).permute(0, 3, 1, 2).double()
    assert float(losses.loss_value(x, y, "boundary")) <= 0.0
    assert float(losses.loss_value(x, y, "hausdorff dt")) < 1e-12


def test_mapping_form():
    x = torch.randn(2, 3, 6, 7, dtype=torch.float64)
    y = blobs(2, 6, 7, 3, 11)
    spec = {"dice": 1.0, "boundary": 0.01, "hausdorff dt": 1e-3}
    loss, grad = losses.loss_and_grad(x, y, spec)
    parts = [losses.loss_and_grad(x, y, n) for n in spec]
    want_l = sum(w * l for w, (l, _) in zip(spec.values(), parts))
    want_g = sum(w * g for w, (_, g) in zip(spec.values(), parts))
    assert abs(float(loss - want_l)) < 1e-14 and float((grad - want_g).abs().max()) < 1e-14


def test_names():
    assert "boundary" in losses.LOSS_NAMES and "hausdorff dt" in losses.LOSS_NAMES
    for spec in ("boundary", "hausdorff dt", {"dice": 1.0, "boundary": 0.01}):
        terms, _ = losses.parse_loss_type(spec, None, 4)
        assert terms
        with pytest.raises(ValueError, match="2 classes"):
            losses.parse_loss_type(spec if isinstance(spec, str) else {"boundary": 1.0}, None, 1)
    x1, y1 = torch.zeros(1, 1, 3, 3), torch.zeros(1, 3, 3, dtype=torch.long)
    for name in ("boundary", "hausdorff dt"):
        with pytest.raises(ValueError):
            losses.loss_and_grad(x1, y1, name)
    for name in ("hausdorff", "contour_smooth", "cross_entropy", "nope", {"boundary": 1.0, "hausdorff": 1.0}):
        with pytest.raises(NotImplementedError):
            losses.parse_loss_type(name, None, 4)
