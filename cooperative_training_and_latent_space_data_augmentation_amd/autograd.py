"""torch.autograd bridge: one Function per *network pass* (not per layer) plus the fused loss / STN-input ops, so the
reference's `loss.backward()` call pattern works unchanged while every FLOP runs in the HIP kernels."""
from __future__ import annotations

import torch

from . import ops
from ._ffi import LOSS_DICE, LOSS_FG_DICE, CtlError
from .consistency import check_kinds as check_consistency_kinds
from .losses import DIST_LOSS_FORM, LOSS_KINDS, check_constant, check_names, check_two_classes, class_weight_tuple, mask_u8, needs_fields
from .recon import check_params as check_recon_params, parse_kinds as parse_recon_kinds


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.float().contiguous(memory_format=torch.channels_last)


def _logit_label(logit, label):
    """What the label-map losses save and their kernels read: fp32 NHWC logits and a contiguous int64 label map."""
    return _nhwc(logit), label.long().contiguous()


class _NetFn(torch.autograd.Function):
    """A whole encoder / decoder pass.  Inputs: the activation `x` and the network's flat parameter buffer."""

    @staticmethod
    def forward(ctx, net, mode, affine, groups, x, flat):
        outs, act, plan = net.run_forward(x, mode, groups)
        net.remember_pass(x, act, outs, plan, mode, groups)
        net._pass_seq += 1
        ctx.counted = bool(flat.requires_grad)            # this pass owes the network a parameter gradient
        if ctx.counted:
            net._pending_bwd += 1
        ctx.net, ctx.mode, ctx.affine, ctx.act, ctx.plan, ctx.seq = net, mode, affine, act, plan, net._pass_seq
        ctx.save_for_backward(x, *outs)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *douts):
        if ctx.mode == "C":
            raise CtlError("backward through an eval-mode (running-statistics) pass is not part of the hot path")
        saved = ctx.saved_tensors
        x, outs = saved[0], saved[1:]
        need_dx, need_w = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        if all(d is None for d in douts) or not (need_dx or need_w):
            return None, None, None, None, None, None
        douts = tuple(None if d is None else _nhwc(d) for d in douts)
        dx, gflat = ctx.net.run_backward(x, ctx.act, outs, ctx.plan, ctx.mode, douts, need_dx, need_w, ctx.affine)
        if gflat is not None and ctx.net._defer_grads:
            # parked for ONE accumulation per network after backward (CtlNet.collect_deferred_grads): handing it to autograd would make
            # every pass a cross-stream dependency on the leaf's accumulation stream when the step runs as two launch chains
            ev = torch.cuda.Event()
            ev.record()
            ctx.net._deferred.append((ctx.seq, gflat, ev))
            gflat = None
        if ctx.counted and need_w:
            net = ctx.net
            net._pending_bwd -= 1
            if net._pending_bwd == 0 and net._on_grads_complete is not None and net._defer_grads and \
                    (net._stack is None or net._stack.done or not net._stack.filled):
                # the last backward pass of this network in this step: its gradient range is complete once the parked per-pass
                # gradients are added; dist.DataParallel does that here, on this pass' stream, and starts the exchange of the range behind it
                net._on_grads_complete()
        return None, None, None, None, dx, gflat


class _SlotFn(torch.autograd.Function):
    """A network pass that is one slot of a PassStack (nets.py): the forward runs now, into the stacked arena; the backward node only
    RECORDS the gradients arriving at the pass' outputs.  The solver issues the stacked backward of all slots once every slot has its
    gradients (CtlNet.backward_stack) and hands the input gradients back to autograd from the pass' input tensors."""

    @staticmethod
    def forward(ctx, net, stack, mode, groups, x, flat):
        p = stack.filled
        outs, act, plan = net.run_forward(x, mode, groups, stack=stack)
        net.remember_pass(x, act, outs, plan, mode, groups)
        net._pass_seq += 1
        stack.seqs.append(net._pass_seq)
        stack.need_dx.append(bool(ctx.needs_input_grad[4]))
        ctx.stack, ctx.p = stack, p
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *douts):
        if all(d is None for d in douts):      # (a sweep that reaches this node without a gradient for it: nothing to record)
            return None, None, None, None, None, None
        if ctx.stack.done:
            raise CtlError("a stacked pass received a gradient after its backward had been issued")
        ctx.stack.receive(ctx.p, douts)
        return None, None, None, None, None, None


def net_apply(net, x: torch.Tensor, groups: int = 1):
    """Run `net` on `x` (logical NCHW) in its current BatchNorm mode; returns a tuple of outputs.  groups > 1: `x` stacks that
    many independent batches along n and BatchNorm handles each as its own call (one launch chain instead of `groups`)."""
    ops.require_gpu(x)
    x = _nhwc(x)
    mode = net.bn_mode()
    track_params = torch.is_grad_enabled() and mode != "C" and net.wants_param_grad()
    flat = net._flat if track_params else net._flat.detach()
    stack = net._stack
    if stack is not None and track_params and stack.accepts(x.shape[0], x.shape[2], x.shape[3], groups):
        outs = _SlotFn.apply(net, stack, mode, groups, x, flat)
        stack.roots.append(x)
        return outs
    return _NetFn.apply(net, mode, mode == "A", groups, x, flat)


class _SplitHalves(torch.autograd.Function):
    """(x[:n], x[n:]) of a stacked (grouped) pass.  Plain slicing would do, but its backward builds two zero-filled NCHW tensors of the
    full stacked size, copies a half into each, adds them and leaves the sum for a layout conversion: ~100 us of fills and copies
    per step.  Here the incoming halves are copied straight into one NHWC tensor."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        ctx.meta = (x.shape, x.device)
        n = x.shape[0] // 2
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None
        shape, device = ctx.meta
        n = shape[0] // 2
        g = torch.empty(shape, dtype=torch.float32, device=device, memory_format=torch.channels_last)
        for half, gh in ((g[:n], ga), (g[n:], gb)):
            if gh is None:
                half.zero_()
            else:
                half.copy_(gh)
        return g


def split_halves(x: torch.Tensor):
    return _SplitHalves.apply(x)


class _CrossEntropy2D(torch.autograd.Function):
    """cross_entropy_2D with an integer label map (custom_loss.py:706-740 / model_util.py:104-115)."""

    @staticmethod
    def forward(ctx, logit, label):
        logit = _nhwc(logit)                  # (_logit_label written out: this forward is on the default step's path, which pays for a call)
        label = label.long().contiguous()
        ctx.save_for_backward(logit, label)
        return ops.ce2d_fwd(logit, label)

    @staticmethod
    def backward(ctx, g):
        logit, label = ctx.saved_tensors
        return ops.ce2d_bwd(logit, label, g.float().contiguous()), None


class _PointwiseSegLoss(torch.autograd.Function):
    """'weighted cross entropy' and 'focal' (custom_loss.py:720-740, :222-255): a pixel's loss term depends on its own row only."""

    @staticmethod
    def forward(ctx, logit, label, kind, class_weights, gamma):
        logit, label = _logit_label(logit, label)
        ctx.save_for_backward(logit, label)
        ctx.args = (kind, class_weights, gamma)
        return ops.seg_loss_fwd(logit, label, kind, class_weights, gamma)[0]

    @staticmethod
    def backward(ctx, g):
        logit, label = ctx.saved_tensors
        kind, class_weights, gamma = ctx.args
        return ops.seg_loss_bwd(logit, label, kind, g.float().contiguous(), None, class_weights, gamma), None, None, None, None


class _DiceSegLoss(torch.autograd.Function):
    """'dice' / 'weighted dice' / 'foreground dice' (custom_loss.py:356-396, :434-471): the forward leaves the per-(sample, class)
    coefficient table of the gradient in its scratch, the backward streams once over the logits with it."""

    @staticmethod
    def forward(ctx, logit, label, kind):
        logit, label = _logit_label(logit, label)
        loss, ws = ops.seg_loss_fwd(logit, label, kind)
        ctx.save_for_backward(logit, label, ws)
        ctx.kind = kind
        return loss

    @staticmethod
    def backward(ctx, g):
        logit, label, ws = ctx.saved_tensors
        return ops.seg_loss_bwd(logit, label, ctx.kind, g.float().contiguous(), ws), None, None


class LabelFields:
    """The class fields of ONE label map [B,H,W] in the training forms of ops.class_fields, each computed on first use and kept: the losses
    of a step that compare different predictions with the same labels share them.  `event` orders a consumer on another stream behind
    the launch that wrote a form (the two launch chains of solver.cooperative_step)."""

    def __init__(self, label: torch.Tensor, n_class: int):
        ops.require_gpu(label)
        self.label, self.n_class = label if label.dtype == torch.uint8 else label.long().contiguous(), int(n_class)
        self._forms = {}

    def get(self, form: str) -> torch.Tensor:
        cur = torch.cuda.current_stream()
        if form not in self._forms:
            f = ops.class_fields(self.label, self.n_class, form)
            ev = torch.cuda.Event()
            ev.record(cur)
            self._forms[form] = (f, ev, cur)
        f, ev, stream = self._forms[form]
        if stream != cur:
            cur.wait_event(ev)
            f.record_stream(cur)
        return f

    def get_all(self, loss_type) -> None:
        """Compute, on the current stream, every form the loss name or {name: weight} mapping `loss_type` reads."""
        for form in needs_fields(loss_type):
            self.get(form)


class _DistSegLoss(torch.autograd.Function):
    """'boundary' / 'hausdorff dt' (losses.py): the label's field arrives as an input; 'hausdorff dt' thresholds the prediction and
    transforms it here, once, and the backward treats that field as the constant the published loss makes it."""

    @staticmethod
    def forward(ctx, logit, label, kind, field):
        logit, label = _logit_label(logit, label)
        pred = ops.class_fields(ops.confident_label(logit), logit.shape[1], "squared") if kind == "hausdorff dt" else None
        ctx.kind, ctx.two = kind, pred is not None
        ctx.save_for_backward(*((logit, label, field) + ((pred,) if ctx.two else ())))
        return ops.dist_loss_fwd(logit, label, kind, field, pred)

    @staticmethod
    def backward(ctx, g):
        logit, label, field = ctx.saved_tensors[:3]
        pred = ctx.saved_tensors[3] if ctx.two else None
        return ops.dist_loss_bwd(logit, label, ctx.kind, g.float().contiguous(), field, pred), None, None, None


class _PairLoss(torch.autograd.Function):
    """The weighted sum of the `kinds` of one family between a tensor and a constant second one: the consistency losses of an output and its
    reference (consistency.py) and the image-similarity losses of a prediction and its target (recon.py).  `pair` = the family's (fwd, bwd)
    of ops.py: one fused forward, whose scratch carries what the one backward launch reads (1/R and the Dice coefficient table, resp. the
    'ncc' table and the 'lncc' coefficient maps).  `params`: the keyword arguments of both."""

    @staticmethod
    def forward(ctx, x, ref, mask, pair, kinds, params):
        x, ref = _nhwc(x), _nhwc(ref)
        loss, _, ws = pair[0](x, ref, kinds, mask=mask, **params)
        ctx.save_for_backward(x, ref, ws, *(() if mask is None else (mask,)))
        ctx.args = (pair[1], dict(kinds), dict(params))
        return loss

    @staticmethod
    def backward(ctx, g):
        x, ref, ws, *mask = ctx.saved_tensors
        bwd, kinds, params = ctx.args
        return bwd(x, ref, kinds, g.float().contiguous(), ws, mask=mask[0] if mask else None, **params), None, None, None, None, None


class _AvgPool(torch.autograd.Function):
    """AvgPool2d(2^scale) of logits, window = stride, floor sizes."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale, ctx.hw = scale, (x.shape[2], x.shape[3])
        return ops.avgpool_fwd(_nhwc(x), scale)

    @staticmethod
    def backward(ctx, g):
        return ops.avgpool_bwd(_nhwc(g), ctx.scale, ctx.hw), None


class _AdvBiasField(torch.autograd.Function):
    """x * exp(S(theta)) (adversarial.py): one forward launch; the backward recomputes the field and gives dtheta and dx in two."""

    @staticmethod
    def forward(ctx, x, theta, spacing):
        x, theta = _nhwc(x), theta.float().contiguous()
        ctx.save_for_backward(x, theta)
        ctx.spacing = spacing
        return ops.adv_bias_fwd(x, theta, spacing)

    @staticmethod
    def backward(ctx, g):
        x, theta = ctx.saved_tensors
        dtheta, dx = ops.adv_bias_bwd(_nhwc(g), x, theta, ctx.spacing, need_dx=ctx.needs_input_grad[0])
        return dx, (dtheta if ctx.needs_input_grad[1] else None), None


class _ScaledMSE(torch.autograd.Function):
    """scale * mean((a-b)^2)"""

    @staticmethod
    def forward(ctx, a, b, scale):
        a, b = _nhwc(a), _nhwc(b)
        ctx.save_for_backward(a, b)
        ctx.scale = scale
        return ops.mse_fwd(a, b, scale)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return ops.mse_bwd(a, b, g.float().contiguous(), ctx.scale), None, None


class _SoftmaxT(torch.autograd.Function):
    """softmax(x / T, dim=C) (construct_input, basic_operations.py:129-131)."""

    @staticmethod
    def forward(ctx, x, temperature):
        p = ops.softmax_t_fwd(_nhwc(x), temperature)
        ctx.save_for_backward(p)
        ctx.t = temperature
        return p

    @staticmethod
    def backward(ctx, dp):
        p, = ctx.saved_tensors
        return ops.softmax_t_bwd(p, _nhwc(dp), ctx.t), None


def cross_entropy_2D(logit, label):
    ops.require_gpu(logit, label)
    return _CrossEntropy2D.apply(logit, label)


def segmentation_loss(logit, label, kind, class_weights=None, gamma=2.0, fields=None):
    """One of the fused segmentation losses of losses.LOSS_KINDS / losses.DIST_LOSS_KINDS on logits [B,C,H,W] and a label map [B,H,W].
    `class_weights`: a host sequence of C numbers, used by 'weighted cross entropy' only ('weighted dice' ignores it, as upstream does);
    `gamma`: 'focal' only.  `fields` ('boundary', 'hausdorff dt'): the class fields of `label`, a LabelFields or the fp32 NHWC tensor of
    the form the loss reads (losses.DIST_LOSS_FORM); computed here when absent."""
    if kind in DIST_LOSS_FORM:
        check_two_classes(kind, logit.size(1))
        ops.require_gpu(logit, label)
        if fields is None:
            fields = LabelFields(label, logit.size(1))
        if isinstance(fields, LabelFields):
            fields = fields.get(DIST_LOSS_FORM[kind])
        return _DistSegLoss.apply(logit, label, kind, fields)
    check_names((kind,), LOSS_KINDS, "segmentation loss")
    ops.require_gpu(logit, label)
    if LOSS_KINDS[kind] in (LOSS_DICE, LOSS_FG_DICE):
        return _DiceSegLoss.apply(logit, label, kind)
    return _PointwiseSegLoss.apply(logit, label, kind, class_weight_tuple(class_weights), float(gamma))


def consistency_loss(output, reference, kinds, class_weights=None, mask=None, is_gt=False):
    """sum_name kinds[name] * L_name(output, reference) of the consistency losses of consistency.CONSISTENCY_KINDS, differentiable
    in `output`; the reference is a constant and must not require grad.  `kinds`: {name: weight}; `class_weights`: a host sequence of C
    numbers ('weighted ce' only); `mask`: per pixel, [B,1,H,W] or [B,H,W], nonzero = 1."""
    check_consistency_kinds(kinds, class_weights)
    check_constant(reference, "reference")
    ops.require_gpu(output, reference, mask)
    return _PairLoss.apply(output, reference, mask_u8(mask), (ops.consistency_fwd, ops.consistency_bwd), kinds,
                           dict(class_weights=class_weight_tuple(class_weights), is_gt=bool(is_gt)))


def avg_pool(x, scale):
    """AvgPool2d(2^scale) of [B,C,H,W] logits on the device, differentiable; scale 0 is the identity."""
    if int(scale) == 0:
        return x
    ops.require_gpu(x)
    return _AvgPool.apply(x, int(scale))


def image_similarity_loss(x, t, kinds, weights=None, mask=None, *, beta=1.0 / 9, win=9, zero_mean=True, reduction="mean"):
    """sum_name weight_name * L_name(x, t) of the image-similarity losses of recon.RECON_KINDS, differentiable in the prediction
    `x`; the target `t` ([B,C,H,W] or [1,C,H,W]) is a constant and must not require grad.  `kinds`: a name, names with `weights`, or
    {name: weight}; `mask`: per pixel, [B,1,H,W] or [B,H,W], nonzero = 1, multiplies x and t."""
    kinds = parse_recon_kinds(kinds, weights)
    check_recon_params(kinds, beta, win, reduction, device=True)
    check_constant(t, "target")
    ops.require_gpu(x, t, mask)
    return _PairLoss.apply(x, t, mask_u8(mask), (ops.recon_loss_fwd, ops.recon_loss_bwd), kinds,
                           dict(beta=float(beta), win=win, zero_mean=bool(zero_mean), reduction=reduction))


def adv_bias_field(x, theta, spacing):
    """The image x [N,C,H,W] times the multiplicative bias field of the log-space control grid theta [N,gh,gw] (ops.adv_bias_grid),
    differentiable in both."""
    ops.require_gpu(x, theta)
    return _AdvBiasField.apply(x, theta, int(spacing))


def adv_unit_scale(g, scale, norm="l2"):
    """ops.adv_unit_scale of a detached g: the bounded step of a gradient.  It has no backward (it is used under no_grad)."""
    g = g.detach().float()
    if not (g.is_contiguous() or (g.dim() == 4 and g.is_contiguous(memory_format=torch.channels_last))):
        g = g.contiguous()
    return ops.adv_unit_scale(g, scale, norm)


def scaled_mse(a, b, scale=1.0):
    ops.require_gpu(a, b)
    return _ScaledMSE.apply(a, b, float(scale))


def softmax_t(x, temperature=2.0):
    ops.require_gpu(x)
    return _SoftmaxT.apply(x, float(temperature))
