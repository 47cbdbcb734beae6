"""Latent-space masking API of the reference (medseg/models/model_util.py), backed by the HIP kernels.

Same names and argument meaning as upstream: `mask_latent_code_channel_wise` (:180-255), `mask_latent_code_spatial_wise`
(:258-318), `_disable_tracking_bn_stats` (:414-451), `set_grad` (:163-165), `makeVariable` (:603-618),
`make_one_hot` (:168-177), `cross_entropy_2D` (:104-115).  Extra keyword-only arguments `k` / `soft_noise` inject the
draws that upstream takes from numpy / torch RNGs (parity tests; CUDA-graph style replays).
"""
from __future__ import annotations

import contextlib
from typing import Optional

import numpy as np
import torch

from . import ops
from .autograd import cross_entropy_2D as _ce2d, scaled_mse as _mse, segmentation_loss as _seg_loss


def set_grad(module, requires_grad=False):
    plist = module.param_list() if hasattr(module, "param_list") else module.parameters()      # (cached list of the engine's networks)
    for p in plist:
        p.requires_grad = requires_grad


def makeVariable(tensor, use_gpu=True, type="long", requires_grad=True):
    t = tensor.data
    if type == "long":
        t = t.long()
    elif type == "float":
        t = t.float()
    else:
        raise NotImplementedError
    if use_gpu:
        t = t.cuda()
    return t.detach().requires_grad_(requires_grad) if t.is_floating_point() else t.detach()


def make_one_hot(y, num_classes=4):
    return ops.onehot(y, num_classes)


def cross_entropy_2D(input, target, weight=None, size_average=True):
    if not size_average or target.dim() != 3:
        raise NotImplementedError("only the averaged, label-map form is on the hot path")
    if weight is not None:      # custom_loss.py:732-736; the weights are launch constants: keep them on the host (a device tensor is read back)
        return _seg_loss(input, target, "weighted cross entropy", weight.tolist() if hasattr(weight, "tolist") else weight)
    return _ce2d(input, target)


@contextlib.contextmanager
def _disable_tracking_bn_stats(model):
    """BatchNorm 'mode B': batch statistics, no running-stat update, gamma/beta frozen for this pass."""
    old = model._bn_track
    bn_params = model.__dict__.get("_bn_plist")           # (cached: the module tree is fixed; the walk cost 0.3 ms of host time per step)
    if bn_params is None:
        bn_params = model.__dict__["_bn_plist"] = [p for m in model.modules() if type(m).__name__ == "_BNP" for p in (m.weight, m.bias)]
    model._bn_track = False
    for p in bn_params:
        p.requires_grad_(False)
    try:
        yield
    finally:
        model._bn_track = old
        for p in bn_params:       # upstream restores requires_grad to the saved *track* flag
            p.requires_grad_(bool(old))


def _draw_seed() -> int:
    return int(torch.randint(0, 2 ** 62, (1,)).item())        # host RNG: respects torch.manual_seed, no device sync


REUSE_SALIENCY_FORWARD = True     # see _saliency_grad


def _saliency_grad(code, decoder_function, label, num_classes, loss_type):
    """dL/dz through the (frozen) decoder: forward + dgrad-only backward (model_util.py:202-223).

    Upstream's saliency pass runs `decoder_function(code)` in training mode on the very tensor the standard pass has just decoded
    (model.py:436-447 store z_i / z_s, model.py:491-501 hands them to perturb_latent_code): same input, same weights, same mode -- the same
    activations, the same batch statistics.  If the decoder still remembers that pass (CtlNet.reuse_pass) its activations are re-used:
    the loss gradient w.r.t. the output is formed from the remembered output, the data-gradient-only backward runs on the remembered
    activations, and the second running-statistics update of every BatchNorm is replayed from the saved batch statistics -- bit for
    bit the numbers of running the pass again (tests/test_engine_gpu.py::test_saliency_forward_reuse_is_bitwise), one decoder forward less."""
    reuse = decoder_function.reuse_pass(ops.as_nhwc(code.detach())) if (REUSE_SALIENCY_FORWARD and hasattr(decoder_function, "reuse_pass")) else None
    if reuse is not None and loss_type in ("ce", "mse", "corr"):
        outs, backward, handle = reuse
        out = outs[0]
        one = torch.ones((), device=out.device)
        if loss_type == "ce":
            dout = ops.ce2d_bwd(out, label.long().contiguous(), one)
        else:
            gt = ops.as_nhwc(ops.onehot(label, num_classes) if label.dim() < code.dim() else label)
            dout = ops.mse_bwd(out, gt, one, 1.0) if loss_type == "mse" else gt / float(out.numel())
        grad = backward((dout,))
        decoder_function.replay_running_stats(handle)
        return ops.as_nhwc(code.detach()), grad
    code = ops.as_nhwc(code.detach()).requires_grad_(True)
    with torch.enable_grad():
        out = decoder_function(code)
        if loss_type == "ce":
            loss = _ce2d(out, label)
            grad = torch.autograd.grad(loss, [code])[0]
        else:
            gt = ops.onehot(label, num_classes) if label.dim() < code.dim() else label
            if loss_type == "mse":
                loss = _mse(out, gt, 1.0)
                grad = torch.autograd.grad(loss, [code])[0]
            elif loss_type == "corr":     # d mean(out*gt) / d out = gt / numel
                grad = torch.autograd.grad(out, [code], grad_outputs=ops.as_nhwc(gt) / float(out.numel()))[0]
            else:
                raise NotImplementedError(loss_type)
    return code.detach(), grad


def _mask(latent_code, decoder_function, label, num_classes, percentile, random, loss_type, if_detach, if_soft, mode,
          k, soft_noise):
    ops.require_gpu(latent_code)
    code, grad = _saliency_grad(latent_code, decoder_function, label, num_classes, loss_type)
    n, c, h, w = code.shape
    L = c if mode == 0 else h * w
    if k is None:
        if random:
            percentile = np.random.rand() * percentile
        k = int(L * percentile)
    if if_soft and soft_noise is None:
        soft_noise = ops.uniform((n, L), code.device, _draw_seed())
    # score -> rank-select -> apply in ONE launch (the three-launch path ops.latent_score + ops.latent_mask_apply computes the same bits)
    masked, mask = ops.latent_mask(grad, code, mode, k, soft_noise if if_soft else None)
    if not if_detach:
        masked = latent_code * mask
    if hasattr(decoder_function, "zero_grad"):
        try:
            decoder_function.zero_grad()
        except Exception:
            pass
    return masked, mask


def mask_latent_code_channel_wise(latent_code, decoder_function, label, num_classes=2, percentile=1 / 3.0, random=False,
                                  loss_type="corr", if_detach=True, if_soft=False, *, k: Optional[int] = None,
                                  soft_noise: Optional[torch.Tensor] = None):
    """Mask the top-k channels ranked by the signed mean of dL/dz over H*W; mask [N,C,1,1]."""
    return _mask(latent_code, decoder_function, label, num_classes, percentile, random, loss_type, if_detach, if_soft, 0, k,
                 soft_noise)


def mask_latent_code_spatial_wise(latent_code, decoder_function, label, num_classes, percentile=1 / 3.0, random=False,
                                  loss_type="corr", if_detach=True, if_soft=False, *, k: Optional[int] = None,
                                  soft_noise: Optional[torch.Tensor] = None):
    """Mask the top-k positions ranked by the signed mean of dL/dz over C; mask [N,1,H,W]."""
    return _mask(latent_code, decoder_function, label, num_classes, percentile, random, loss_type, if_detach, if_soft, 1, k,
                 soft_noise)


# ---------------------------------------------------------------------------------------------- EMA of the weights (:21-101)
class ExponentialMovingAverage:
    """Upstream's class on any parameter list, plain torch: shadow <- shadow - (1 - decay_t) * (shadow - param) per update, with
    decay_t = min(decay, (1 + n) / (10 + n)) for update number n when use_num_updates.  (The solver keeps its shadows flat on the device
    and updates them inside the Adam pass -- optim.FlatAdam.ema; this class is the statement those are tested against.)"""

    def __init__(self, parameters, decay, use_num_updates=True):
        if not 0.0 <= decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self.shadow_params = [p.clone().detach() for p in parameters if p.requires_grad]
        self.collected_params = []

    def update(self, parameters):
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = min(decay, (1 + self.num_updates) / (10 + self.num_updates))
        omd = 1.0 - decay
        with torch.no_grad():
            for s, p in zip(self.shadow_params, [p for p in parameters if p.requires_grad]):
                s.sub_(omd * (s - p))

    def copy_to(self, parameters):
        for s, p in zip(self.shadow_params, parameters):
            if p.requires_grad:
                p.data.copy_(s.data)

    def store(self, parameters):
        self.collected_params = [p.clone() for p in parameters if p.requires_grad]

    def restore(self, parameters):
        if not self.collected_params:
            print("did not find any copy, use the original params")
            return
        for c, p in zip(self.collected_params, parameters):
            if p.requires_grad:
                p.data.copy_(c.data)


# ---------------------------------------------------------------------------------------------- learning-rate schedules (:589-671)
def lr_poly(base_lr, iter, max_iter, power):
    return base_lr * ((1 - float(iter) / max_iter) ** power)


def adjust_learning_rate(optimizer, i_iter, initial_learning_rate, total_steps, power=0.985):
    """:593-600: the polynomial rate into every param group; a second group runs at ten times it."""
    lr = lr_poly(initial_learning_rate, i_iter, total_steps, power)
    for group in optimizer.param_groups:
        group["lr"] = lr
    if len(optimizer.param_groups) > 1:
        optimizer.param_groups[1]["lr"] = lr * 10
    return lr


class _FactorSchedule:
    """lr(epoch) = base_lr * factor(epoch), the closed form of torch's LambdaLR / StepLR: the rate of epoch 0 is written at construction,
    step() moves to the next epoch.  Works on anything with `param_groups` (FlatAdam, torch.optim.Optimizer)."""

    def __init__(self, optimizer, factor):
        self.optimizer, self.factor = optimizer, factor
        self.base_lrs = [g["lr"] for g in optimizer.param_groups]
        self.last_epoch = 0
        self._write()

    def _write(self):
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = base * self.factor(self.last_epoch)

    def step(self, metric=None):
        self.last_epoch += 1
        self._write()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"base_lrs": list(self.base_lrs), "last_epoch": self.last_epoch}

    def load_state_dict(self, sd):
        self.base_lrs, self.last_epoch = list(sd["base_lrs"]), int(sd["last_epoch"])
        self._write()


class _PlateauSchedule:
    """torch's ReduceLROnPlateau(mode='min', threshold_mode='rel', cooldown=0, min_lr=0, eps=1e-8): step(metric) multiplies the rate by
    `factor` once the metric has not fallen below best * (1 - threshold) for more than `patience` calls in a row."""

    def __init__(self, optimizer, factor, threshold=0.01, patience=5, eps=1e-8):
        self.optimizer, self.factor, self.threshold, self.patience, self.eps = optimizer, factor, threshold, patience, eps
        self.best, self.num_bad_epochs, self.last_epoch = float("inf"), 0, 0

    def step(self, metric=None):
        if metric is None:
            raise ValueError("a plateau schedule needs the epoch's metric: step(metric)")
        current = float(metric)
        self.last_epoch += 1
        if current < self.best * (1.0 - self.threshold):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            for g in self.optimizer.param_groups:
                old = float(g["lr"])
                new = max(old * self.factor, 0.0)
                if old - new > self.eps:
                    g["lr"] = new
            self.num_bad_epochs = 0

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"best": self.best, "num_bad_epochs": self.num_bad_epochs, "last_epoch": self.last_epoch, "lrs": self.get_last_lr()}

    def load_state_dict(self, sd):
        self.best, self.num_bad_epochs, self.last_epoch = float(sd["best"]), int(sd["num_bad_epochs"]), int(sd["last_epoch"])
        for g, lr in zip(self.optimizer.param_groups, sd["lrs"]):
            g["lr"] = lr


def _warmstart(hi, lo):
    return lambda epoch: 0.1 if epoch < 5 else (1 if epoch < hi else (0.1 if epoch < lo else 0.01))


def get_scheduler(optimizer, lr_policy, lr_decay_iters=5, epoch_count=None, niter=None, niter_decay=None):
    """:621-671, the seven policies as small host objects with `.step(metric=None)` that write `param_groups[*]['lr']`; they restate
    torch's closed forms and need no torch.optim.lr_scheduler (which refuses FlatAdam).  An unknown name raises NotImplementedError
    (upstream returns the exception object)."""
    if lr_policy == "lambda":
        return _FactorSchedule(optimizer, lambda epoch: 1.0 - max(0, epoch + 1 + epoch_count - niter) / float(niter_decay + 1))
    if lr_policy in ("step", "step2"):
        gamma = 0.5 if lr_policy == "step" else 0.1
        return _FactorSchedule(optimizer, lambda epoch: gamma ** (epoch // lr_decay_iters))
    if lr_policy in ("plateau", "plateau2"):
        return _PlateauSchedule(optimizer, factor=0.1 if lr_policy == "plateau" else 0.2, threshold=0.01, patience=5)
    if lr_policy == "step_warmstart":
        return _FactorSchedule(optimizer, _warmstart(100, 200))
    if lr_policy == "step_warmstart2":
        return _FactorSchedule(optimizer, _warmstart(50, 100))
    raise NotImplementedError("learning rate policy [%s] is not implemented" % lr_policy)
