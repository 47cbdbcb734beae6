"""Plain float64 restatements of the element-wise / reduction operations of csrc/ctl_elem.hip: one function per operation, written from
its definition (no autograd inside), NCHW in and out, torch-CPU float64.  tests/test_elem_ref_cpu.py checks every function against
torch.autograd; tests/test_elem_gpu.py checks the HIP kernels against these functions.

BatchNorm groups are independent passes batched along n: group k owns the samples [k * n/groups, (k+1) * n/groups)."""
import torch

F64 = torch.float64


def f64(t):
    return t.detach().to("cpu", F64)


def rb(t):
    """round to bf16 (round-to-nearest-even), back to float64"""
    return t.detach().float().to(torch.bfloat16).to(F64)


def _bc(v, n, groups):
    """[groups, c] coefficients -> [n, c, 1, 1], sample i reads group i // (n / groups)"""
    gi = torch.arange(n) // (n // groups)
    return v.reshape(groups, -1)[gi].reshape(n, -1, 1, 1)


def leaky(z, slope):
    return torch.where(z > 0, z, z * slope)


def leaky_grad(z, slope):
    """derivative factor chosen from the sign of z: 1 where z > 0, slope elsewhere (z == 0 included)"""
    return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))


# ------------------------------------------------------------------------------------------------ BatchNorm forward
def bn_finalize(x, gamma, beta, eps, momentum, running_mean=None, running_var=None, nbt=0, groups=1, update_running=True):
    """Statistics of every group of x and the running update over the groups in order.  Returns a dict of [groups, c] tensors mean, var
    (biased), uvar (unbiased), invstd, scale, shift and the final running_mean, running_var [c] and nbt."""
    x = f64(x)
    n, c = x.shape[:2]
    per = n // groups
    count = per * x.shape[2] * x.shape[3]
    mean, var, uvar = (torch.empty(groups, c, dtype=F64) for _ in range(3))
    rm = None if running_mean is None else f64(running_mean).clone()
    rv = None if running_var is None else f64(running_var).clone()
    for k in range(groups):
        xs = x[k * per:(k + 1) * per]
        mean[k] = xs.sum((0, 2, 3)) / count
        var[k] = ((xs - mean[k].view(1, -1, 1, 1)) ** 2).sum((0, 2, 3)) / count
        uvar[k] = var[k] * count / (count - 1) if count > 1 else var[k]
        if update_running:
            rm = (1 - momentum) * rm + momentum * mean[k]
            rv = (1 - momentum) * rv + momentum * uvar[k]
            nbt += 1
    invstd = 1 / torch.sqrt(var + eps)
    scale = f64(gamma).view(1, -1) * invstd
    shift = f64(beta).view(1, -1) - mean * scale
    return dict(mean=mean, var=var, uvar=uvar, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv, nbt=nbt)


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps, groups=1):
    """inference-mode coefficients, the same row for every group"""
    sc = f64(gamma) / torch.sqrt(f64(running_var) + eps)
    sh = f64(beta) - f64(running_mean) * sc
    return sc.repeat(groups, 1), sh.repeat(groups, 1)


def bn_act(x, scale, shift, slope, groups=1):
    x = f64(x)
    n = x.shape[0]
    return leaky(x * _bc(f64(scale), n, groups) + _bc(f64(shift), n, groups), slope)


def bn_replay_running(running_mean, running_var, nbt, mean, uvar, momentum):
    """one more running update from saved batch statistics"""
    return ((1 - momentum) * f64(running_mean) + momentum * f64(mean), (1 - momentum) * f64(running_var) + momentum * f64(uvar), nbt + 1)


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def bwd_g(mode, dy, act_src=None, u=None, scale=None, shift=None, slope=0.2, groups=1):
    """the gradient behind the activation: mode 0 dy * leaky'(act_src) (also the `ds` output), mode 1 dy * leaky'(u * scale + shift),
    mode 2 dy"""
    dy = f64(dy)
    if mode == 0:
        return dy * leaky_grad(f64(act_src), slope)
    if mode == 1:
        n = dy.shape[0]
        return dy * leaky_grad(f64(u) * _bc(f64(scale), n, groups) + _bc(f64(shift), n, groups), slope)
    return dy


def bwd_sums(g, u=None, groups=1):
    """[groups, c] sums of g and of g * u (mode 2: the sum of g only, u = None)"""
    n, c = g.shape[:2]
    gg = g.reshape(groups, n // groups, c, -1)
    s1 = gg.sum((1, 3))
    if u is None:
        return s1, None
    return s1, (gg * f64(u).reshape(groups, n // groups, c, -1)).sum((1, 3))


def bwd_coefs(s1, s2, count, gamma, mean, invstd):
    """dx = A*g + B*u + C of the BatchNorm backward, from dx = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)), xhat = (u-mean)*invstd.
    Returns A, B, C, sum_g, sum_gxhat, each [groups, c]."""
    mean, invstd = f64(mean).reshape(s1.shape), f64(invstd).reshape(s1.shape)
    gam = f64(gamma).view(1, -1)
    sum_g = s1
    sum_gxhat = invstd * (s2 - mean * s1)
    m1, m2 = sum_g / count, sum_gxhat / count
    A = gam * invstd
    B = -gam * invstd * invstd * m2
    C = -gam * invstd * m1 + gam * invstd * invstd * m2 * mean
    return A.expand_as(s1).clone(), B, C, sum_g, sum_gxhat


def bwd_dparams(sum_g, sum_gxhat, dgamma0=None, dbeta0=None, accumulate=False, affine_groups=0):
    """dgamma / dbeta: the groups whose bit is set in affine_groups (0 = every group) summed, on top of the previous value with accumulate"""
    groups, c = sum_g.shape
    dgamma = f64(dgamma0).clone() if accumulate else torch.zeros(c, dtype=F64)
    dbeta = f64(dbeta0).clone() if accumulate else torch.zeros(c, dtype=F64)
    for k in range(groups):
        if affine_groups == 0 or (affine_groups >> k) & 1:
            dgamma = dgamma + sum_gxhat[k]
            dbeta = dbeta + sum_g[k]
    return dgamma, dbeta


def bwd_apply(g, u, A, B, C, groups=1):
    n = g.shape[0]
    return _bc(A, n, groups) * g + _bc(B, n, groups) * f64(u) + _bc(C, n, groups)


def sumpool2(x):
    x = f64(x)
    return x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]


def accumulate(dst, srcs):
    out = f64(dst).clone()
    for s in srcs:
        out = out + f64(s)
    return out


# ------------------------------------------------------------------------------------------------ STN builders, losses
def softmax_t_fwd(x, temperature):
    z = f64(x) / temperature
    e = torch.exp(z - z.max(1, keepdim=True)[0])
    return e / e.sum(1, keepdim=True)


def softmax_t_bwd(p, dp, temperature):
    p, dp = f64(p), f64(dp)
    return p * (dp - (p * dp).sum(1, keepdim=True)) / temperature


def onehot(label, c):
    """[n, h, w] integer labels -> [n, c, h, w]"""
    return (label.cpu().long().unsqueeze(1) == torch.arange(c).view(1, c, 1, 1)).to(F64)


def _log_softmax(x):
    z = f64(x)
    z = z - z.max(1, keepdim=True)[0]
    return z - torch.log(torch.exp(z).sum(1, keepdim=True))


def ce_mean(x, label):
    return float(-(_log_softmax(x) * onehot(label, x.shape[1])).sum() / label.numel())


def ce_grad(x, label, gout=1.0):
    return float(gout) / label.numel() * (torch.exp(_log_softmax(x)) - onehot(label, x.shape[1]))


def mse(a, b, scale=1.0):
    return float(scale * ((f64(a) - f64(b)) ** 2).sum() / a.numel())


def mse_grad(a, b, gout=1.0, scale=1.0):
    return float(gout) * 2.0 * scale / a.numel() * (f64(a) - f64(b))


def sigmoid_bwd(dy, y):
    y = f64(y)
    return f64(dy) * y * (1 - y)


def argmax_first(x):
    """index of the first maximum over the channels (numpy.argmax order), uint8"""
    x = f64(x)
    best, idx = x[:, 0].clone(), torch.zeros(x[:, 0].shape, dtype=torch.uint8)
    for k in range(1, x.shape[1]):
        hit = x[:, k] > best
        best = torch.where(hit, x[:, k], best)
        idx = torch.where(hit, torch.full_like(idx, k), idx)
    return idx


# ------------------------------------------------------------------------------------------------ Adam
def adam(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """torch.optim.Adam without amsgrad / weight decay on the gradient g * grad_scale; bias corrections in float64.  Returns p, m, v."""
    g = f64(g) * grad_scale
    m = beta1 * f64(m) + (1 - beta1) * g
    v = beta2 * f64(v) + (1 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = torch.sqrt(v) / (bc2 ** 0.5) + eps
    return f64(p) - (lr / bc1) * (m / denom), m, v


# ------------------------------------------------------------------------------------------------ comparison
def rel_err(a, ref, per_channel=False, bf16_out=False):
    """max over the elements of |a - ref| / norm.  norm is max|ref| over the whole tensor, or with per_channel the channel's own max|ref|
    (4-d: dim 1 is the channel; otherwise every element is its own channel), floored at 1e-6.  bf16_out takes one bf16 rounding of the
    stored result, |ref| * 2^-8, off the error first."""
    a, ref = f64(a), f64(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    err = (a - ref).abs()
    if bf16_out:
        err = (err - ref.abs() * 2.0 ** -8).clamp_min(0)
    if per_channel:
        norm = ref.abs().amax((0, 2, 3), keepdim=True) if ref.dim() == 4 else ref.abs()
    else:
        norm = ref.abs().max()
    if not torch.isfinite(a).all():
        return float("inf")
    return float((err / norm.clamp_min(1e-6)).max())


def close(a, ref, rel, what="", per_channel=False, bf16_out=False):
    e = rel_err(a, ref, per_channel, bf16_out)
    assert e <= rel, f"{what}: relative error {e:.3e} > {rel:.3e}" + (" (per channel)" if per_channel else "")
    return e
