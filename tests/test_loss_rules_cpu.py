"""One statement per rule of the loss families: every layer that accepts an argument (the public function, the host statement, the autograd
wrapper, the ops *_fwd / *_bwd pair) refuses a bad one with the same exception class and the same rule text, before it looks at the tensors
(these are CPU tensors: a layer that looked at them first would raise the "device tensors" error instead).  And every family states its
name -> library kind table once: the *_NAMES tuple is the table's keys, the values are the constants of include/ctl_hip.h in header order."""
import re

import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, autograd, consistency as K, losses, ops, recon, solver

X, R = torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8)
Y = torch.zeros(2, 8, 8, dtype=torch.long)
XI, TI = torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8)
ONE, WS = torch.ones(()), torch.zeros(8, dtype=torch.float64)


def refuses(err, text, calls):
    for call in calls:
        with pytest.raises(err, match=re.escape(text)):
            call()


def cons_layers(kinds, cw=None, r=R):
    """Every layer of the consistency family on one {name: weight} mapping."""
    names, weights = list(kinds), list(kinds.values())
    return [lambda: K.calc_segmentation_consistency(X, r, names, weights, cw), lambda: K.consistency_and_grad(X, r, names, weights, cw),
            lambda: autograd.consistency_loss(X, r, kinds, cw), lambda: ops.consistency_fwd(X, r, kinds, cw),
            lambda: ops.consistency_bwd(X, r, kinds, ONE, WS, cw)]


def recon_layers(kinds, t=TI, host=True, **kw):
    """Every layer of the image-similarity family; host=False leaves out the two that take CPU tensors as they are."""
    device = [lambda: autograd.image_similarity_loss(XI, t, kinds, **kw), lambda: ops.recon_loss_fwd(XI, t, kinds, **kw),
              lambda: ops.recon_loss_bwd(XI, t, kinds, ONE, WS, **kw)]
    return ([lambda: recon.image_similarity(XI, t, kinds, **kw), lambda: recon.similarity_and_grad(XI, t, kinds, **kw)] if host else []) + device


def test_unknown_names():
    refuses(NotImplementedError, "consistency loss 'dice' (one of kl, ce, weighted ce, mse, Dice, contour)", cons_layers({"kl": 1.0, "dice": 1.0}))
    refuses(NotImplementedError, "image-similarity loss 'ssim' (one of mse, l1, smooth l1, ncc, lncc)", recon_layers({"mse": 1.0, "ssim": 1.0}))
    refuses(NotImplementedError, "segmentation loss 'nope' (one of ",
            [lambda: solver.basic_loss_fn(X, Y, "nope"), lambda: solver.basic_loss_fn(X, Y, {"dice": 1.0, "nope": 1.0}),
             lambda: losses.loss_and_grad(X, Y, "nope"), lambda: autograd.segmentation_loss(X, Y, "nope"),
             lambda: ops.seg_loss_fwd(X, Y, "nope"), lambda: ops.seg_loss_bwd(X, Y, "nope", ONE)])
    refuses(NotImplementedError, "distance-map loss 'hausdorff' (one of boundary, hausdorff dt)",
            [lambda: ops.dist_loss_fwd(X, Y, "hausdorff", X, X), lambda: ops.dist_loss_bwd(X, Y, "hausdorff", ONE, X, X)])


def test_empty_kinds():
    refuses(ValueError, "consistency loss: no names (`kinds` maps at least one name to its weight)", cons_layers({}))
    refuses(ValueError, "image-similarity loss: no names (`kinds` maps at least one name to its weight)", recon_layers({}))
    refuses(ValueError, "segmentation loss: no names (`kinds` maps at least one name to its weight)",
            [lambda: solver.basic_loss_fn(X, Y, {}), lambda: losses.loss_and_grad(X, Y, {})])


def test_weights():
    for bad in (float("nan"), float("inf"), float("-inf")):
        refuses(ValueError, f"the weight of 'l1' is {bad} (finite)",
                [lambda: recon.image_similarity(XI, TI, {"mse": 1.0, "l1": bad}), lambda: recon.similarity_and_grad(XI, TI, ["mse", "l1"], [1.0, bad]),
                 lambda: autograd.image_similarity_loss(XI, TI, {"l1": bad})])
    refuses(ValueError, "'weighted ce' must be given class weights", cons_layers({"kl": 1.0, "weighted ce": 1.0}))
    # one weight per class: the layers that know the class count before they look at the tensors' device
    refuses(ValueError, "each class must have a weight: expected 4 weights, got 3",
            cons_layers({"weighted ce": 1.0}, [1.0, 2.0, 3.0])[:2] +
            [lambda: solver.basic_loss_fn(X, Y, "weighted cross entropy", [1.0, 2.0, 3.0]), lambda: solver.basic_loss_fn(X, Y, "dice", torch.ones(3)),
             lambda: losses.loss_and_grad(X, Y, "weighted cross entropy", [1.0, 2.0, 3.0]), lambda: losses.normalised_weights((1, 2, 3), 4)])
    assert losses.class_weight_tuple(torch.tensor([1, 2, 3, 4]), 4) == losses.class_weight_tuple([1, 2.0, 3, 4]) == (1.0, 2.0, 3.0, 4.0)
    assert losses.class_weight_tuple(None, 4) is None


def test_image_similarity_parameters():
    refuses(ValueError, "reduction 'batch' ('mean' or 'sum')", recon_layers({"mse": 1.0}, reduction="batch"))
    for beta in (0.0, -0.5):
        refuses(ValueError, f"beta = {beta} (smooth l1 needs beta > 0)", recon_layers({"smooth l1": 1.0}, beta=beta))
    for win in (4, 1, 17):
        refuses(ValueError, f"win = {win} (the window size win_size: odd, 3 .. 15)",
                recon_layers({"lncc": 1.0}, win=win) + [lambda: recon.CustomLocalNormalizedCrossCorrelationLoss(win_size=win)])
    refuses(NotImplementedError, "reduction='none' is not offered on the device ('mean' or 'sum'; CPU tensors take 'none')",
            recon_layers({"mse": 1.0}, host=False, reduction="none"))
    refuses(ValueError, "reduction 'none' ('mean' or 'sum')", [lambda: recon.similarity_and_grad(XI, TI, "mse", reduction="none")])
    assert recon.image_similarity(XI, TI, "mse", reduction="none").shape == XI.shape                  # the CPU path offers it


def test_the_second_tensor_is_a_constant():
    refuses(ValueError, "the reference is a constant: detach it (no gradient reaches the reference)",
            cons_layers({"kl": 1.0}, r=R.clone().requires_grad_(True))[:3])
    refuses(ValueError, "the target is a constant: detach it (no gradient reaches the target)",
            recon_layers({"mse": 1.0}, t=TI.clone().requires_grad_(True))[:3])


def test_mask_conversions():
    m = torch.tensor([[0, 7], [255, 0]], dtype=torch.uint8).expand(2, 2, 2).contiguous()
    for mask in (m, m.reshape(2, 1, 2, 2), m.float() * -0.5, m.bool(), m.long()):
        assert torch.equal(losses.mask01(mask, (2, 3, 2, 2), torch.float64, "cpu"), (m != 0).double().reshape(2, 1, 2, 2))      # nonzero = 1
        u8 = losses.mask_u8(mask)
        assert u8.dtype == torch.uint8 and u8.is_contiguous() and u8.shape == mask.shape and torch.equal(u8 != 0, m.reshape(mask.shape) != 0)
    assert losses.mask_u8(m) is m and losses.mask_u8(None) is None               # the kernels take every nonzero byte as 1
    assert torch.equal(losses.mask01(None, (2, 3, 2, 2), torch.float32, "cpu"), torch.ones(2, 1, 2, 2))
    for bad in (torch.ones(2, 2, 8, 8), torch.ones(1, 1, 8, 8), torch.ones(2, 8, 7)):
        refuses(ValueError, "the mask is per pixel: [2,1,8,8] or [2,8,8], got",
                [lambda: K.calc_segmentation_consistency(X, R, mask=bad), lambda: K.consistency_and_grad(X, R, mask=bad),
                 lambda: recon.image_similarity(XI, TI, "mse", mask=bad), lambda: recon.similarity_and_grad(XI, TI, "mse", mask=bad)])


def test_one_table_per_family():
    f = _ffi
    for table, names, values in (
            (losses.LOSS_KINDS, losses.LOSS_NAMES[1:6], (f.LOSS_WCE, f.LOSS_FOCAL, f.LOSS_DICE, f.LOSS_DICE, f.LOSS_FG_DICE)),
            (losses.DIST_LOSS_KINDS, losses.DIST_LOSS_NAMES, (f.DLOSS_BOUNDARY, f.DLOSS_HAUSDORFF_DT)),
            (K.CONSISTENCY_KINDS, K.CONSISTENCY_NAMES, (f.CONS_KL, f.CONS_CE, f.CONS_WCE, f.CONS_MSE, f.CONS_DICE, f.CONS_CONTOUR)),
            (recon.RECON_KINDS, recon.RECON_NAMES, (f.RECON_MSE, f.RECON_L1, f.RECON_SMOOTH_L1, f.RECON_NCC, f.RECON_LNCC))):
        assert tuple(table) == tuple(names) and tuple(table.values()) == values
        assert list(values) == sorted(values)                                                           # header order
    assert losses.LOSS_NAMES == ("cross entropy",) + tuple(losses.LOSS_KINDS) + losses.DIST_LOSS_NAMES  # 'cross entropy': no fused kind
    assert losses.LOSS_KINDS["weighted dice"] == f.LOSS_DICE
    assert tuple(losses.DIST_LOSS_FORM) == losses.DIST_LOSS_NAMES
    # the binding layer holds no table of its own
    assert ops.LOSS_KINDS is losses.LOSS_KINDS and ops.DIST_LOSS_KINDS is losses.DIST_LOSS_KINDS and ops.DIST_LOSS_FORM is losses.DIST_LOSS_FORM
    assert ops.CONSISTENCY_KINDS is K.CONSISTENCY_KINDS and ops.RECON_KINDS is recon.RECON_KINDS


def test_one_needs_fields():
    assert losses.needs_fields("boundary") == ["signed"] and losses.needs_fields({"hausdorff dt": 1.0, "dice": 1.0, "boundary": 0.1}) == ["squared", "signed"]
    assert losses.needs_fields("cross entropy") == [] and losses.needs_fields({"dice": 1.0, "focal": 1.0}) == []
    assert solver.needs_fields({"dice": 1.0, "boundary": 0.1}) is True and solver.needs_fields("dice") is False
