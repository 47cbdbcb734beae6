"""Host statements of the optimizer tail (no GPU): model_util.ExponentialMovingAverage and the seven get_scheduler policies against
tests/golden/optim_cases.pt (recorded from upstream's own classes by tools/gen_golden_optim.py) and against live torch schedulers;
optim.adam_tail_host / grad_norm_host, the definitions the kernels are tested against; FlatAdam's state dicts with and without EMA."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, model_util, nets, optim
from oracle import ref_elem as R

GOLD = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_cases.pt"))
POLICIES = ["lambda", "step", "step2", "plateau", "plateau2", "step_warmstart", "step_warmstart2"]


class _Stub:
    """what the schedulers need of FlatAdam: param_groups"""

    def __init__(self, lr, groups=1):
        self.param_groups = [{"lr": lr, "params": []} for _ in range(groups)]


def _real(lr):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=lr)


# ---------------------------------------------------------------------------------------------- EMA
@pytest.mark.parametrize("case", GOLD["ema"], ids=lambda c: f"{c['dtype']}-{'warmup' if c['use_num_updates'] else 'fixed'}")
def test_ema_equals_upstreams_shadows_bit_for_bit(case):
    params = [torch.nn.Parameter(t.clone()) for t in case["start"]]
    ema = model_util.ExponentialMovingAverage(params, case["decay"], use_num_updates=case["use_num_updates"])
    assert (ema.num_updates == 0) if case["use_num_updates"] else (ema.num_updates is None)
    for n, feed in enumerate(case["feed"], 1):
        with torch.no_grad():
            for p, f in zip(params, feed):
                p.copy_(f)
        ema.update(params)
        if n in case["shadows"]:
            for s, want in zip(ema.shadow_params, case["shadows"][n]):
                assert s.dtype == want.dtype and torch.equal(s, want), (n, (s - want).abs().max())
    assert ema.num_updates == (30 if case["use_num_updates"] else None)


def test_ema_fp32_statement_of_adam_tail_host_is_the_class():
    """The EMA half of adam_tail_host (what the kernel is held to) is the class's arithmetic on fp32 tensors, omd from num_updates."""
    case = next(c for c in GOLD["ema"] if c["dtype"] == "float32" and c["use_num_updates"])
    shadow = [t.clone() for t in case["start"]]
    z = [torch.zeros_like(t) for t in case["start"]]
    for n, feed in enumerate(case["feed"][:3], 1):
        omd = 1.0 - optim.ema_decay_at(case["decay"], n)
        # lr = 0: the Adam half leaves p = feed, so the shadow sees exactly the fed parameters
        shadow = [optim.adam_tail_host(f, zz, zz, zz + 1.0, s, 0.0, (0.9, 0.999), 1e-8, n, omd=omd)[3] for f, zz, s in zip(feed, z, shadow)]
    for s, want in zip(shadow, case["shadows"][3]):
        assert torch.equal(s, want)


def test_ema_store_copy_to_restore_round_trip():
    params = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]
    ema = model_util.ExponentialMovingAverage(params, 0.9)
    with torch.no_grad():
        for p in params:
            p.add_(1.0)
    ema.update(params)
    live = [p.detach().clone() for p in params]
    ema.store(params)
    ema.copy_to(params)
    for p, s, l in zip(params, ema.shadow_params, live):
        assert torch.equal(p, s) and not torch.equal(p, l)
    ema.restore(params)
    for p, l in zip(params, live):
        assert torch.equal(p, l)
    with pytest.raises(ValueError):
        model_util.ExponentialMovingAverage(params, 1.5)


# ---------------------------------------------------------------------------------------------- schedules
def _run(sch, opt, case):
    lrs = [opt.param_groups[0]["lr"]]
    for i in range(len(case["lrs"]) - 1):
        sch.step(case["metrics"][i] if case["metrics"] is not None else None)
        lrs.append(opt.param_groups[0]["lr"])
    return lrs


@pytest.mark.parametrize("make", [lambda lr: _Stub(lr), _real], ids=["flatadam-like", "torch-adam"])
@pytest.mark.parametrize("case", GOLD["sched"], ids=lambda c: c["policy"] + "".join(f"-{v}" for v in c["kwargs"].values()))
def test_schedules_equal_upstreams_sequences(case, make):
    assert 8 <= len(case["lrs"]) - 1 <= 210
    opt = make(case["base_lr"])
    sch = model_util.get_scheduler(opt, case["policy"], **case["kwargs"])
    got = _run(sch, opt, case)
    assert len(set(case["lrs"])) > 1                     # every recorded series moves
    for i, (a, b) in enumerate(zip(got, case["lrs"])):
        assert abs(a - b) <= 1e-12 * abs(b), (case["policy"], i, a, b)
    assert sch.get_last_lr() == [got[-1]]


def test_every_policy_is_recorded_and_unknown_names_raise():
    assert {c["policy"] for c in GOLD["sched"]} == set(POLICIES)
    lam = next(c for c in GOLD["sched"] if c["policy"] == "lambda")
    assert lam["kwargs"] == dict(epoch_count=0, niter=3, niter_decay=4)
    with pytest.raises(NotImplementedError):
        model_util.get_scheduler(_Stub(1e-4), "cosine")


@pytest.mark.parametrize("policy", POLICIES)
def test_schedules_equal_a_live_torch_scheduler(policy):
    from torch.optim import lr_scheduler as L
    kw = dict(epoch_count=1, niter=4, niter_decay=6) if policy == "lambda" else (dict(lr_decay_iters=3) if policy.startswith("step") else {})
    ours_opt, ref_opt = _real(3e-4), _real(3e-4)
    ours = model_util.get_scheduler(ours_opt, policy, **kw)
    warm = lambda hi, lo: (lambda e: 0.1 if e < 5 else (1 if e < hi else (0.1 if e < lo else 0.01)))      # noqa: E731
    ref = {"lambda": lambda: L.LambdaLR(ref_opt, lambda e: 1.0 - max(0, e + 1 + 1 - 4) / float(6 + 1)),
           "step": lambda: L.StepLR(ref_opt, step_size=3, gamma=0.5), "step2": lambda: L.StepLR(ref_opt, step_size=3, gamma=0.1),
           "plateau": lambda: L.ReduceLROnPlateau(ref_opt, mode="min", factor=0.1, threshold=0.01, patience=5),
           "plateau2": lambda: L.ReduceLROnPlateau(ref_opt, mode="min", factor=0.2, threshold=0.01, patience=5),
           "step_warmstart": lambda: L.LambdaLR(ref_opt, warm(100, 200)), "step_warmstart2": lambda: L.LambdaLR(ref_opt, warm(50, 100))}[policy]()
    metric = [1.0 / (1 + i) if i < 4 else 0.25 for i in range(230)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(30 if "plateau" in policy else (12 if policy in ("lambda", "step", "step2") else 210)):
            assert abs(ours_opt.param_groups[0]["lr"] - ref_opt.param_groups[0]["lr"]) <= 1e-12 * abs(ref_opt.param_groups[0]["lr"]), (policy, i)
            ref_opt.step()
            if "plateau" in policy:
                ours.step(metric[i]); ref.step(metric[i])      # noqa: E702
            else:
                ours.step(); ref.step()                        # noqa: E702
    assert ours_opt.param_groups[0]["lr"] != 3e-4 or policy == "lambda"


def test_scheduler_state_round_trips_and_plateau_needs_a_metric():
    for policy in ("step", "plateau2"):
        a_opt, b_opt = _Stub(1e-3), _Stub(1e-3)
        a, b = model_util.get_scheduler(a_opt, policy, lr_decay_iters=2), model_util.get_scheduler(b_opt, policy, lr_decay_iters=2)
        for i in range(9):
            a.step(1.0)
        b.load_state_dict(a.state_dict())
        for i in range(9):
            a.step(1.0); b.step(1.0)                           # noqa: E702
            assert a_opt.param_groups[0]["lr"] == b_opt.param_groups[0]["lr"] < 1e-3
    with pytest.raises(ValueError):
        model_util.get_scheduler(_Stub(1e-3), "plateau").step()


def test_lr_poly_and_adjust_learning_rate():
    for base, it, mx, power, want in GOLD["poly"]:
        assert model_util.lr_poly(base, it, mx, power) == want
    opt = _Stub(1.0, groups=2)
    lr = model_util.adjust_learning_rate(opt, 37, 1e-4, 100)
    assert lr == model_util.lr_poly(1e-4, 37, 100, 0.985)
    assert opt.param_groups[0]["lr"] == lr and opt.param_groups[1]["lr"] == lr * 10


# ---------------------------------------------------------------------------------------------- Adam tail / norm statements
def test_adam_tail_host_with_neutral_settings_is_the_oracles_adam():
    g = torch.Generator().manual_seed(3)
    p, gr, m = (torch.randn(1000, generator=g) for _ in range(3))
    v = torch.rand(1000, generator=g)
    for step, scale in ((1, 1.0), (2, 0.5), (1000, 0.125)):
        want = R.adam(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, step, scale)
        got = optim.adam_tail_host(p, gr, m, v, None, 1e-3, (0.9, 0.999), 1e-8, step, grad_scale=scale, clip=1.0)
        for a, b in zip(got[:3], want):
            assert a.dtype == torch.float64 and torch.equal(a, b)
        assert got[3] is None
    clipped = optim.adam_tail_host(p, gr, m, v, None, 1e-3, (0.9, 0.999), 1e-8, 1, clip=0.25)
    assert torch.equal(clipped[1], R.adam(p, gr * 0.25, m, v, 1e-3, 0.9, 0.999, 1e-8, 1)[1])


def test_grad_norm_host_against_fsum():
    g = torch.Generator().manual_seed(4)
    grads = [torch.randn(n, generator=g) * s for n, s in ((1, 1.0), (4097, 1e-3), (70001, 30.0))]
    exact = math.fsum(float(x) * float(x) for t in grads for x in t.tolist())
    n = sum(t.numel() for t in grads)
    for scale in (1.0, 0.5, 0.125):
        sumsq, norm, clip, finite = optim.grad_norm_host(grads, scale, 0.0, False)
        assert abs(sumsq - exact) <= n * 2.0 ** -53 * exact and finite and clip == 1.0
        assert abs(norm - scale * math.sqrt(exact)) <= n * 2.0 ** -53 * norm
        for max_norm in (norm * 0.5, norm, norm * 4):
            c = optim.grad_norm_host(grads, scale, max_norm, True)[2]
            assert c == min(1.0, max_norm / (norm + 1e-6)) and (c < 1.0) == (max_norm <= norm)
    for bad in (float("nan"), float("inf")):
        grads[1][5] = bad
        sumsq, norm, clip, finite = optim.grad_norm_host(grads, 1.0, 1.0, True)
        assert not finite and clip == 1.0 and not math.isfinite(norm)


# ---------------------------------------------------------------------------------------------- FlatAdam state
def _net():
    return nets.build_networks(device="cpu")["segmentation_decoder"]


def test_flat_adam_state_dict_is_unchanged_without_ema():
    net = _net()
    plain, routed = optim.FlatAdam(net, lr=1e-4), optim.FlatAdam(net, lr=1e-4)
    routed.configure(torch.zeros(_ffi.OPTIM_CTRL_DOUBLES, dtype=torch.float64), 3, use_ema=False)
    for o in (plain, routed):
        o.step_count = 2
        o.exp_avg.fill_(0.5)
    a, b = plain.state_dict(), routed.state_dict()
    assert list(a) == list(b) == ["state", "param_groups"] and routed.ema is None and routed.net_index == 3
    assert a["param_groups"] == b["param_groups"] and list(a["param_groups"][0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "params"]
    assert a["state"].keys() == b["state"].keys()
    for i in a["state"]:
        assert list(a["state"][i]) == list(b["state"][i]) == ["step", "exp_avg", "exp_avg_sq"]
        assert all(torch.equal(a["state"][i][k], b["state"][i][k]) for k in a["state"][i])


def test_flat_adam_ema_state_round_trips_and_old_files_load(tmp_path):
    net = _net()
    opt = optim.FlatAdam(net, lr=1e-4)
    old = opt.state_dict()                                 # a file written before the tail existed
    opt.configure(torch.zeros(_ffi.OPTIM_CTRL_DOUBLES, dtype=torch.float64), 0, use_ema=True)
    assert torch.equal(opt.ema, net._flat_data) and opt.ema.data_ptr() != net._flat_data.data_ptr() and opt.num_updates == 0
    opt.step_count, opt.num_updates = 4, 4
    opt.ema.mul_(0.5)
    opt.exp_avg.fill_(0.25)
    torch.save(opt.state_dict(), tmp_path / "o.pth")
    sd = torch.load(tmp_path / "o.pth")
    assert set(sd) == {"state", "param_groups", "ema", "num_updates"} and sd["num_updates"] == 4
    assert [tuple(e.shape) for e in sd["ema"]] == [tuple(p.shape) for p in net.parameters()]
    other = optim.FlatAdam(_net(), lr=1e-4)
    other.configure(torch.zeros(_ffi.OPTIM_CTRL_DOUBLES, dtype=torch.float64), 0, use_ema=True)
    other.load_state_dict(sd)
    assert other.num_updates == 4 and other.step_count == 4
    assert all(torch.equal(a, b) for a, b in zip(other._views(other.exp_avg), opt._views(opt.exp_avg)))      # (views: the padding is not state)
    for a, b in zip(other._views(other.ema), opt._views(opt.ema)):
        assert torch.equal(a, b)
    other.load_state_dict(old)                             # no EMA keys: the shadow restarts from the weights
    assert other.num_updates == 0 and torch.equal(other.ema, other.net._flat_data)
    plain = optim.FlatAdam(_net(), lr=1e-4)
    plain.load_state_dict(sd)                              # EMA keys, EMA off here: ignored
    assert plain.ema is None and plain.step_count == 4


def test_ema_decay_rule():
    assert optim.ema_decay_at(0.999, None) == 0.999
    assert [optim.ema_decay_at(0.999, n) for n in (1, 2, 3)] == [2 / 11, 3 / 12, 4 / 13]
    assert optim.ema_decay_at(0.5, 100) == 0.5
    assert np.float32(1.0 - optim.ema_decay_at(0.999, 10 ** 6)) == np.float32(1.0 - 0.999)
