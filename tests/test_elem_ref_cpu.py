"""oracle/ref_elem.py is the reference tests/test_elem_gpu.py holds the element-wise HIP kernels to.  Here every function of it is checked
against torch.autograd in float64 (F.batch_norm, F.leaky_relu, F.cross_entropy, F.mse_loss, torch.softmax, torch.optim.Adam,
F.avg_pool2d * 4), at small shapes, without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_elem as R

F64 = torch.float64
TOL = 1e-11


def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _grouped_bn(u, gamma, beta, rm, rv, groups, eps=1e-5, momentum=0.1):
    per = u.shape[0] // groups
    return torch.cat([F.batch_norm(u[k * per:(k + 1) * per], rm, rv, gamma, beta, True, momentum, eps) for k in range(groups)])


@pytest.mark.parametrize("n,c,h,w,groups", [(2, 4, 3, 5, 1), (4, 8, 5, 3, 2), (6, 3, 2, 2, 3), (1, 8, 3, 3, 1)])
def test_bn_finalize_and_apply_match_batch_norm(n, c, h, w, groups):
    g = torch.Generator().manual_seed(n + c)
    u = torch.randn(n, c, h, w, generator=g, dtype=F64) * 1.5 + 0.7
    gamma, beta = torch.rand(c, generator=g, dtype=F64) + 0.5, torch.randn(c, generator=g, dtype=F64)
    rm, rv = torch.randn(c, generator=g, dtype=F64), torch.rand(c, generator=g, dtype=F64) + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    ref = F.leaky_relu(_grouped_bn(u, gamma, beta, rm_t, rv_t, groups), 0.2)
    st = R.bn_finalize(u, gamma, beta, 1e-5, 0.1, rm, rv, nbt=5, groups=groups)
    assert rel(st["running_mean"], rm_t) < TOL and rel(st["running_var"], rv_t) < TOL and st["nbt"] == 5 + groups
    assert rel(R.bn_act(u, st["scale"], st["shift"], 0.2, groups), ref) < TOL
    per = n // groups
    for k in range(groups):
        uk = u[k * per:(k + 1) * per]
        assert rel(st["mean"][k], uk.mean((0, 2, 3))) < TOL
        assert rel(st["var"][k], uk.var((0, 2, 3), unbiased=False)) < TOL
        assert rel(st["uvar"][k], uk.var((0, 2, 3), unbiased=True)) < TOL
        assert rel(st["invstd"][k], 1 / torch.sqrt(uk.var((0, 2, 3), unbiased=False) + 1e-5)) < TOL
    # without the running update the buffers come back as they went in
    st0 = R.bn_finalize(u, gamma, beta, 1e-5, 0.1, rm, rv, nbt=5, groups=groups, update_running=False)
    assert torch.equal(st0["running_mean"], rm) and torch.equal(st0["running_var"], rv) and st0["nbt"] == 5
    # evaluation mode: running statistics, the same row for every group
    sc, sh = R.bn_eval_coeffs(gamma, beta, rm, rv, 1e-5, groups)
    ev = F.leaky_relu(F.batch_norm(u, rm.clone(), rv.clone(), gamma, beta, False, 0.1, 1e-5), 0.2)
    assert sc.shape == (groups, c) and rel(R.bn_act(u, sc, sh, 0.2, groups), ev) < TOL
    # the replay is one more running update from the saved statistics
    rm2, rv2, nbt2 = R.bn_replay_running(rm, rv, 7, st["mean"][0], st["uvar"][0], 0.1)
    rm_r, rv_r = rm.clone(), rv.clone()
    F.batch_norm(u[:per], rm_r, rv_r, gamma, beta, True, 0.1, 1e-5)
    assert rel(rm2, rm_r) < TOL and rel(rv2, rv_r) < TOL and nbt2 == 8


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,c,h,w,groups", [(2, 4, 3, 5, 1), (4, 8, 5, 3, 2), (6, 4, 2, 3, 3), (1, 8, 3, 3, 1)])
def test_bn_backward_identity_matches_autograd(mode, n, c, h, w, groups):
    """mode 1: a = leaky(BN(u)); mode 0: out = leaky(r + BN(u)) (the residual tail, ds = dL/dr).  dx = A*g + B*u + C equals autograd's
    input gradient to 1e-11, dgamma / dbeta (all groups, one group only, on top of an earlier value) the parameter gradients."""
    g = torch.Generator().manual_seed(10 * mode + n + c)
    u = (torch.randn(n, c, h, w, generator=g, dtype=F64) * 1.5 + 0.7).requires_grad_(True)
    r = torch.randn(n, c, h, w, generator=g, dtype=F64, requires_grad=True)
    gammas = [(torch.rand(c, generator=g, dtype=F64) + 0.5).requires_grad_(True) for _ in range(groups)]
    betas = [torch.randn(c, generator=g, dtype=F64, requires_grad=True) for _ in range(groups)]
    dy = torch.randn(n, c, h, w, generator=g, dtype=F64)
    per = n // groups
    # every group with parameters of its own (same values): autograd then yields the per-group parameter gradients
    with torch.no_grad():
        for k in range(1, groups):
            gammas[k].copy_(gammas[0]); betas[k].copy_(betas[0])
    bn = torch.cat([F.batch_norm(u[k * per:(k + 1) * per], None, None, gammas[k], betas[k], True, 0.1, 1e-5) for k in range(groups)])
    out = F.leaky_relu(bn + r if mode == 0 else bn, 0.2)
    out.backward(dy)
    st = R.bn_finalize(u, gammas[0], betas[0], 1e-5, 0.1, groups=groups, update_running=False)
    gg = R.bwd_g(mode, dy, act_src=out, u=u, scale=st["scale"], shift=st["shift"], slope=0.2, groups=groups)
    if mode == 0:
        assert rel(gg, r.grad) < TOL                       # ds
    s1, s2 = R.bwd_sums(gg, u, groups)
    A, B, C, sum_g, sum_gx = R.bwd_coefs(s1, s2, per * h * w, gammas[0], st["mean"], st["invstd"])
    assert rel(R.bwd_apply(gg, u, A, B, C, groups), u.grad) < TOL
    dg_all, db_all = R.bwd_dparams(sum_g, sum_gx)
    assert rel(dg_all, sum(x.grad for x in gammas)) < TOL and rel(db_all, sum(x.grad for x in betas)) < TOL
    for k in range(groups):
        d0, b0 = torch.randn(c, generator=g, dtype=F64), torch.randn(c, generator=g, dtype=F64)
        dg, db = R.bwd_dparams(sum_g, sum_gx, d0, b0, accumulate=True, affine_groups=1 << k)
        assert rel(dg, d0 + gammas[k].grad) < TOL and rel(db, b0 + betas[k].grad) < TOL
        dg, db = R.bwd_dparams(sum_g, sum_gx, d0, b0, accumulate=False, affine_groups=1 << k)
        assert rel(dg, gammas[k].grad) < TOL and rel(db, betas[k].grad) < TOL
    # mode 2: plain channel sums
    s, none = R.bwd_sums(R.bwd_g(2, dy))
    assert none is None and rel(s[0], dy.sum((0, 2, 3))) < TOL


def test_sumpool_accumulate_sigmoid_onehot_argmax():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 6, 10, generator=g, dtype=F64)
    assert rel(R.sumpool2(x), F.avg_pool2d(x, 2) * 4) < TOL
    # sum-pool is the gradient of nearest upsampling
    z = torch.randn(2, 4, 3, 5, generator=g, dtype=F64, requires_grad=True)
    F.interpolate(z, scale_factor=2, mode="nearest").backward(x)
    assert rel(R.sumpool2(x), z.grad) < TOL
    srcs = [torch.randn(37, generator=g, dtype=F64) for _ in range(5)]
    assert rel(R.accumulate(srcs[0], srcs[1:]), torch.stack(srcs).sum(0)) < TOL
    a = torch.randn(3, 1, 4, 5, generator=g, dtype=F64, requires_grad=True)
    y = torch.sigmoid(a)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)
    assert rel(R.sigmoid_bwd(dy, y), a.grad) < TOL
    lab = torch.randint(0, 7, (3, 4, 5), generator=g)
    assert torch.equal(R.onehot(lab, 7), F.one_hot(lab, 7).permute(0, 3, 1, 2).to(F64))
    t = torch.randint(-2, 3, (3, 5, 4, 6), generator=g).to(F64)          # many exact ties
    assert np.array_equal(R.argmax_first(t).numpy(), np.argmax(t.numpy(), axis=1).astype(np.uint8))
    assert int(R.argmax_first(torch.zeros(1, 4, 2, 2)).max()) == 0


@pytest.mark.parametrize("c", [1, 2, 4, 7, 16])
@pytest.mark.parametrize("scale", [3.0, 200.0])
def test_softmax_and_losses_match_autograd(c, scale):
    g = torch.Generator().manual_seed(c)
    x = (torch.randn(3, c, 5, 4, generator=g, dtype=F64) * scale).requires_grad_(True)
    lab = torch.randint(0, c, (3, 5, 4), generator=g)
    p = torch.softmax(x / 2, dim=1)
    dp = torch.randn(p.shape, generator=g, dtype=F64)
    p.backward(dp)
    assert rel(R.softmax_t_fwd(x, 2.0), p) < TOL
    if c > 1:
        assert rel(R.softmax_t_bwd(p, dp, 2.0), x.grad) < 1e-9            # (autograd's own cancellation at saturated rows)
    x.grad = None
    loss = F.cross_entropy(x, lab)
    (loss * 0.7).backward()
    assert abs(R.ce_mean(x, lab) - float(loss)) <= TOL * max(1.0, abs(float(loss)))
    if c > 1:
        assert rel(R.ce_grad(x, lab, 0.7), x.grad) < TOL
    a = torch.rand(3, c, 5, 4, generator=g, dtype=F64, requires_grad=True)
    b = torch.rand(3, c, 5, 4, generator=g, dtype=F64)
    l2 = 0.5 * F.mse_loss(a, b)
    (l2 * 1.3).backward()
    assert abs(R.mse(a, b, 0.5) - float(l2)) < TOL and rel(R.mse_grad(a, b, 1.3, 0.5), a.grad) < TOL
    assert R.mse(a, a, 0.5) == 0.0 and float(R.mse_grad(a, a).abs().max()) == 0.0


@pytest.mark.parametrize("grad_scale", [1.0, 0.5, 0.125])
def test_adam_matches_torch_optim(grad_scale):
    g = torch.Generator().manual_seed(2)
    p = torch.randn(101, generator=g, dtype=F64)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    m, v = torch.zeros(101, dtype=F64), torch.zeros(101, dtype=F64)
    for step in range(1, 6):
        gr = torch.randn(101, generator=g, dtype=F64)
        ref.grad = gr * grad_scale
        opt.step()
        p, m, v = R.adam(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, step, grad_scale)
        assert rel(p, ref.detach()) < TOL
        st = opt.state[ref]
        assert rel(m, st["exp_avg"]) < TOL and rel(v, st["exp_avg_sq"]) < TOL


def test_rb_and_comparison_helpers():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.14159, 1e-3])
    assert torch.equal(R.rb(t), t.to(torch.bfloat16).double())
    assert float(R.rb(torch.tensor([1.0 + 2.0 ** -8]))) == 1.0 and float(R.rb(torch.tensor([1.0 + 3 * 2.0 ** -8]))) == 1.0 + 2.0 ** -6   # ties to even
    ref = torch.tensor([1000.0, 1.0])
    bad = torch.tensor([1000.0, 1.01])                     # the small channel is 1 % off
    R.close(bad, ref, 1e-4, "whole tensor")                # hidden by the large one under the whole-tensor norm
    with pytest.raises(AssertionError):
        R.close(bad, ref, 1e-4, "per channel", per_channel=True)
    r4 = torch.ones(2, 2, 3, 3); r4[:, 0] *= 1000
    b4 = r4.clone(); b4[0, 1, 1, 1] = 1.01
    R.close(b4, r4, 1e-4)
    with pytest.raises(AssertionError):
        R.close(b4, r4, 1e-4, per_channel=True)
    # one bf16 rounding of the stored result is allowed only with bf16_out
    x = torch.tensor([3.14159, -2.71828])
    R.close(R.rb(x), x, 1e-7, bf16_out=True)
    with pytest.raises(AssertionError):
        R.close(R.rb(x), x, 1e-7)
    with pytest.raises(AssertionError):
        R.close(torch.tensor([float("nan"), 1.0]), torch.tensor([1.0, 1.0]), 1.0)
    assert R.rel_err(torch.zeros(3), torch.zeros(3), per_channel=True) == 0.0           # floor 1e-6, no division by zero
