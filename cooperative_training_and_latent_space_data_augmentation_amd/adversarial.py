"""Adversarial input augmentation: the two input-space baselines the paper compares latent-space masking against, adversarial noise
("Adv Noise", VAT-style) and an adversarial multiplicative bias field ("Adv Bias").  A project addition: upstream has no counterpart, so
the float64 host statement below is the definition the kernels (csrc/ctl_adv.hip) are tested against.  DESIGN.md lists the deviations.

Bias field.  Plane H x W, integer control-point spacing s >= 2, grid gh = (H - 1) // s + 4, gw = (W - 1) // s + 4, parameters theta
[n, gh, gw] in log space.  For pixel row y: i = y // s, t = (y - i s) / s, columns alike, and
    S(y, x) = sum_{a,b = 0..3} B_a(t_y) B_b(t_x) theta[i_y + a, i_x + b],   B0 = (1 - t)^3 / 6,  B1 = (3 t^3 - 6 t^2 + 4) / 6,
                                                                           B2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6,  B3 = t^3 / 6:
the approximating uniform cubic B-spline, no prefilter.  The weights are non-negative and sum to 1, so |S| <= max |theta|.  The field is
f = exp(S) and x' = x f, the same field for every channel.  The constraint is on theta: clamped to [log(1 - eps), log(1 + eps)] it gives
1 - eps <= f <= 1 + eps on every pixel.  Adjoint, given g = dL/dx':  dL/dS = f sum_c g_c x_c,  dL/dtheta = My^T (dL/dS) Mx with M the
[H, gh] / [W, gw] weight matrices (`bias_weights`),  dL/dx = g f.
Noise.  x' = x + delta, delta [n, C, H, W]; no clamp, the map stays linear; dL/ddelta = g.
Unit step, per sample: 'l2' scale g / ||g||_2, 'rms' scale g / sqrt(mean g^2), 'linf' scale g / max |g|; a sample whose norm is 0 or not
finite gives zeros.
Generation (`generate`), VAT-style with K = power_iterations: the reference prediction comes from the clean image under no_grad; start
at p0 = xi unit(r), r uniform in (-1, 1) from the counter-hash generator (ops.uniform, seeded); K times: x' = T(x; p), the fast network
on x' without tracking BatchNorm statistics, the 'kl' consistency against the constant reference (with labels: the solver's own
segmentation loss), the gradient with respect to p only, the step -- noise: delta = eps unit_rms(grad); bias: theta = clamp(log(1 + eps)
unit_linf(grad)).  Returns T(x; p) detached, and p.

Device tensors run the HIP kernels in fp32; CPU tensors take the same arithmetic from torch ops in their own dtype."""
from __future__ import annotations

import math

import torch

NORMS = ("l2", "rms", "linf")


# ---------------------------------------------------------------------------------------------- the host statement (float64)
def bias_grid(h: int, w: int, s: int):
    if int(s) != s or s < 2:
        raise ValueError(f"spacing = {s} (an integer >= 2)")
    if h < 1 or w < 1:
        raise ValueError(f"plane {h}x{w}")
    return (int(h) - 1) // int(s) + 4, (int(w) - 1) // int(s) + 4


def bias_weights(L: int, s: int) -> torch.Tensor:
    """M [L, (L - 1) // s + 4], float64: M[y, y // s + a] = B_a((y - (y // s) s) / s), zero elsewhere."""
    g = bias_grid(L, L, s)[0]
    y = torch.arange(L, dtype=torch.int64)
    i = y // int(s)
    t = (y - i * int(s)).double() / float(s)
    t2, t3 = t * t, t * t * t
    B = torch.stack([(1.0 - t) ** 3 / 6.0, (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0, (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0, t3 / 6.0], 1)
    M = torch.zeros(L, g, dtype=torch.float64)
    for a in range(4):
        M[y, i + a] = B[:, a]
    return M


def _check_bias(x, theta, s):
    if x.dim() != 4 or theta.dim() != 3:
        raise ValueError("expected an image [n,C,H,W] and a control grid [n,gh,gw]")
    n, _, h, w = x.shape
    if tuple(theta.shape) != (n,) + bias_grid(h, w, s):
        raise ValueError(f"a {h}x{w} plane at spacing {s} has a control grid {bias_grid(h, w, s)}, got {tuple(theta.shape[1:])} for {n} samples")


def bias_field_host(x, theta, s):
    """(x', f): float64 CPU tensors [n,C,H,W] and [n,H,W]."""
    _check_bias(x, theta, s)
    xd, th = x.detach().double().cpu(), theta.detach().double().cpu()
    My, Mx = bias_weights(xd.shape[2], s), bias_weights(xd.shape[3], s)
    f = torch.exp(torch.einsum("ya,nab,xb->nyx", My, th, Mx))
    return xd * f.unsqueeze(1), f


def bias_field_grad_host(g, x, theta, s):
    """(dL/dtheta [n,gh,gw], dL/dx [n,C,H,W]) for g = dL/dx', float64, in closed form."""
    _check_bias(x, theta, s)
    gd, xd = g.detach().double().cpu(), x.detach().double().cpu()
    My, Mx = bias_weights(xd.shape[2], s), bias_weights(xd.shape[3], s)
    f = bias_field_host(x, theta, s)[1]
    dS = f * (gd * xd).sum(1)
    return torch.einsum("ya,nyx,xb->nab", My, dS, Mx), gd * f.unsqueeze(1)


def _norm(flat, norm):
    if norm == "l2":
        return flat.pow(2).sum(1).sqrt()
    if norm == "rms":
        return flat.pow(2).mean(1).sqrt()
    if norm == "linf":
        return flat.abs().amax(1)
    raise ValueError(f"norm {norm!r} (one of {', '.join(NORMS)})")


def _unit_scale_torch(g, scale, norm):
    flat = g.reshape(g.shape[0], -1)
    r = _norm(flat, norm)
    ok = torch.isfinite(r) & (r > 0)
    shape = (-1,) + (1,) * (g.dim() - 1)
    out = float(scale) * g / torch.where(ok, r, torch.ones_like(r)).view(shape)
    return torch.where(ok.view(shape), out, torch.zeros_like(out))


def unit_scale_host(g, scale, norm="l2"):
    """Per sample (first axis) scale g / norm(g) in float64; zeros for a sample whose norm is 0 or not finite."""
    return _unit_scale_torch(g.detach().double().cpu(), scale, norm)


# ---------------------------------------------------------------------------------------------- the perturbation models
def unit_scale(g, scale, norm="l2"):
    """The unit step on the device (two launches) or, for a CPU tensor, from torch ops in its dtype."""
    if norm not in NORMS:
        raise ValueError(f"norm {norm!r} (one of {', '.join(NORMS)})")
    if g.is_cuda:
        from . import autograd
        return autograd.adv_unit_scale(g, scale, norm)
    return _unit_scale_torch(g.detach(), scale, norm)


def _hash_uniform(shape, like, seed):
    """uniform in (-1, 1): the counter-hash generator on the device; a seeded torch generator for a CPU tensor"""
    if like.is_cuda:
        from . import ops
        return ops.uniform(tuple(shape), like.device, int(seed)) * 2.0 - 1.0
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64).to(like.dtype) * 2.0 - 1.0


class AdvNoise:
    """Additive adversarial noise of rms radius `epsilon` (default: the sigma of the Gaussian input noise of the training loop)."""
    kind = "noise"

    def __init__(self, epsilon=0.05, xi=1e-2, power_iterations=1):
        if not (epsilon > 0 and xi > 0) or int(power_iterations) != power_iterations or power_iterations < 0:
            raise ValueError("AdvNoise: epsilon > 0, xi > 0, power_iterations an integer >= 0")
        self.epsilon, self.xi, self.power_iterations = float(epsilon), float(xi), int(power_iterations)

    def init(self, image, seed):
        n, c, h, w = image.shape
        r = _hash_uniform((n, h, w, c), image, seed).permute(0, 3, 1, 2)          # drawn in memory (NHWC) order
        return unit_scale(r, self.xi, "rms")

    def apply(self, image, p):
        return image + p

    def step(self, p, grad):
        return unit_scale(grad, self.epsilon, "rms")

    def project(self, p):
        return p


class AdvBias:
    """Multiplicative adversarial bias field within [1 - epsilon, 1 + epsilon] from a control grid at `spacing` pixels."""
    kind = "bias"

    def __init__(self, epsilon=0.3, spacing=32, xi=1e-1, power_iterations=1):
        if not (0 < epsilon < 1 and xi > 0) or int(power_iterations) != power_iterations or power_iterations < 0:
            raise ValueError("AdvBias: 0 < epsilon < 1, xi > 0, power_iterations an integer >= 0")
        if int(spacing) != spacing or spacing < 2:
            raise ValueError(f"AdvBias: spacing = {spacing} (an integer >= 2)")
        self.epsilon, self.spacing, self.xi, self.power_iterations = float(epsilon), int(spacing), float(xi), int(power_iterations)
        self.lo, self.hi = math.log(1.0 - self.epsilon), math.log(1.0 + self.epsilon)

    def init(self, image, seed):
        n, _, h, w = image.shape
        r = _hash_uniform((n,) + bias_grid(h, w, self.spacing), image, seed)
        return self.project(unit_scale(r, self.xi, "linf"))

    def apply(self, image, p):
        if image.is_cuda:
            from . import autograd
            return autograd.adv_bias_field(image, p, self.spacing)
        _check_bias(image, p, self.spacing)
        My = bias_weights(image.shape[2], self.spacing).to(image.dtype)
        Mx = bias_weights(image.shape[3], self.spacing).to(image.dtype)
        return image * torch.exp(torch.einsum("ya,nab,xb->nyx", My, p.to(image.dtype), Mx)).unsqueeze(1)

    def step(self, p, grad):
        return self.project(unit_scale(grad, self.hi, "linf"))

    def project(self, p):
        return p.clamp(self.lo, self.hi)


KINDS = {"noise": AdvNoise, "bias": AdvBias}


def make_chain(kind="bias", **params):
    """The transforms of `kind`: a name, or a tuple of names (bias first, then noise); `params`: {name: {constructor arguments}} or, for a
    single name, its constructor arguments directly."""
    names = (kind,) if isinstance(kind, str) else tuple(kind)
    if not names or len(set(names)) != len(names) or any(k not in KINDS for k in names):
        raise ValueError(f"kind {kind!r}: 'bias', 'noise' or a tuple of the two")
    if len(names) == 1 and not (set(params) <= set(KINDS)):
        params = {names[0]: params}
    unknown = set(params) - set(names)
    if unknown:
        raise ValueError(f"parameters for {sorted(unknown)}, which {kind!r} does not name")
    return tuple(KINDS[k](**params.get(k, {})) for k in sorted(names))                # 'bias' < 'noise'


def generate(solver, image, label=None, chain=None, seed=0):
    """(x_adv, [p per transform]) by the loop of the module docstring.  `chain`: transforms (default: one AdvBias); a chain of both kinds
    applies the bias first, then the noise, and takes the two gradients in the same backward.  The solver must be in train() mode (the
    backward of an eval-mode pass is not offered); its requires_grad flags, gradients and BatchNorm running buffers are left as they were."""
    from .autograd import consistency_loss
    from .model_util import set_grad
    nets = None if not getattr(solver, "training", False) else [solver.model["image_encoder"], solver.model["segmentation_decoder"]]
    if nets is None or not all(net.training for net in nets):               # (solver.eval() leaves solver.training set, as upstream does)
        raise RuntimeError("adversarial generation needs the solver in train() mode: the backward through an eval-mode pass is not offered")
    chain = (AdvBias(),) if chain is None else tuple(sorted(chain, key=lambda t: t.kind))
    if not chain or len({t.kind for t in chain}) != len(chain):
        raise ValueError("chain: one transform, or one AdvBias and one AdvNoise")
    iters = {t.power_iterations for t in chain}
    if len(iters) != 1:
        raise ValueError("the transforms of a chain share one backward per iteration: give them the same power_iterations")
    flags = [[p.requires_grad for p in net.param_list()] for net in nets]
    image = image.detach()

    def transformed(ps):
        x = image
        for t, p in zip(chain, ps):
            x = t.apply(x, p)
        return x

    try:
        with torch.no_grad():
            params = [t.init(image, int(seed) + i) for i, t in enumerate(chain)]
            y_ref = None if label is not None else solver.fast_predict(image, disable_track_bn_stats=True)[1].detach()
        fields = None if label is None else solver._label_fields(label)
        for _ in range(iters.pop()):
            for net in nets:                          # (a pass without BatchNorm tracking hands gamma / beta their flag back: set again)
                set_grad(net, False)
            ps = [p.detach().requires_grad_(True) for p in params]
            y = solver.fast_predict(transformed(ps), disable_track_bn_stats=True)[1]
            loss = consistency_loss(y, y_ref, {"kl": 1.0}) if label is None else solver._seg_loss(y, label, fields)
            grads = torch.autograd.grad(loss, ps)
            with torch.no_grad():
                params = [t.step(p, g) for t, p, g in zip(chain, params, grads)]
        with torch.no_grad():
            x_adv = transformed(params)
    finally:
        for net, fl in zip(nets, flags):
            for p, v in zip(net.param_list(), fl):
                p.requires_grad = v
    return x_adv.detach(), params
