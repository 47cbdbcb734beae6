"""The EXECUTION FORMS of the bf16 engine (compute_dtype="bf16", BASELINE config 3): graph replay (runtime / segments), two launch chains,
saliency-forward re-use, split graph with a gradient hook, optimizer tail under replay, whole-volume inference, checkpoint resume, grouped
BatchNorm passes.  tests/test_graph_gpu.py, tests/test_engine_gpu.py and tests/test_optim_solver_gpu.py pin these forms for the fp32
engine; the bf16 engine differs in orchestration exactly there (solver.split_backward off, virtual dV / dU staged from (g, BatchNorm
input, coefficients) until the deferred stacked weight gradients, the bf16 bit of the batched weight re-pack, grouped STN passes by
default), so every statement is made again on bf16 solvers.

Every kernel of the step is deterministic (no float atomics, ordered two-stage sums): a form is THE SAME computation as the plain eager
step, and items 1-8 compare with torch.equal -- losses of every step, flat weights, BatchNorm buffers and num_batches_tracked, Adam
moments and step counts (`_state` / `_same` of tests/test_graph_gpu.py), masks where named, the next np.random draw where the host
draws.  Grouped passes (item 9) change the order of the statistics partials and are compared with the rounding-point oracle
(oracle/bf16_plan.py, oracle.ref_cpu.bf16_rounding_points) within the bounds tests/test_bf16_engine_gpu.py and
tests/test_bf16_backward_gpu.py already state; no tolerance is introduced here.

Shapes: 4 x 64^2 for the step tests (the smallest bf16 step the suite already ran), 2 x 64^2 where the fp32 original uses it (the golden
cases C / D / E are 2 x 64^2), 2 x 32^2 for the optimizer tail (the bf16 plans of all five networks compile at that size, so the tail test
uses the shape of its fp32 original), the network inputs of tests/test_bf16_engine_gpu.py::NET_INPUT for the grouped passes."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import bf16_plan as P  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, nets  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.graph import CooperativeStepGraph  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.model_util import _disable_tracking_bn_stats  # noqa: E402
import test_bf16_backward_gpu as TBB  # noqa: E402
import test_bf16_engine_gpu as TB  # noqa: E402
import test_engine_gpu as TE  # noqa: E402
import test_optim_solver_gpu as TO  # noqa: E402
from test_graph_gpu import CH_MSE, CH_MSE_RT, DROP_CE, DROP_MSE, SP_CE, SP_CE_RT, _same, _state, dev  # noqa: E402
from test_graph_gpu import _solver as _graph_solver  # noqa: E402

DEV = "cuda"


def _solver(golden_sd):
    return _graph_solver(golden_sd, "bf16")


def _batch(n, h, w, seed):
    return tuple(dev(t) for t in O.synthetic_batch(n, h, w, seed=seed))


def _losses(l):
    return torch.stack([v.detach().float() for v in l]).cpu()


def _launches():
    return int(_ffi.lib.ctl_launch_count())


def _differs(a, b):
    """names of the parts of two `_state` tuples that are not bit-identical"""
    bad = []
    for k in a[0]:
        if not torch.equal(a[0][k], b[0][k]):
            bad.append(f"weights of {k}")
        if not (torch.equal(a[1][k][0], b[1][k][0]) and torch.equal(a[1][k][1], b[1][k][1])):
            bad.append(f"BatchNorm buffers of {k}")
        if not (torch.equal(a[2][k][0], b[2][k][0]) and torch.equal(a[2][k][1], b[2][k][1]) and a[2][k][2] == b[2][k][2]):
            bad.append(f"Adam state of {k}")
    return bad


# ---------------------------------------------------------------------------------------------- 1. graph replay is the eager step
@pytest.mark.parametrize("replay", ["runtime", "segments"])
@pytest.mark.parametrize("cfgs", [(CH_MSE, SP_CE), (CH_MSE_RT, SP_CE_RT)], ids=["fixed_k", "random_k"])
@pytest.mark.parametrize("two_streams", [True, False])
def test_bf16_graph_replay_is_bitwise_the_eager_step(golden_sd, cfgs, two_streams, replay):
    """4 bf16 training steps, eager vs graph replay, from the same weights and the same seeded host RNG.  Then `predict(noisy)` of both
    (it reads the PACKED bf16 weights: a replay that did not carry the bf16 re-pack trains on stale packs), then one further eager step on
    both.  Everything is collected before anything is asserted, so that a failure names every comparison that broke.
    Node-count floor of the segment graphs: every library launch of the step is a kernel node of the captured graph (torch's own kernels
    come on top), so the graph holds at least the launches the eager bf16 step of this test was counted to make."""
    clean, label, noisy = _batch(4, 64, 64, seed=5)
    res = []
    for use_graph in (False, True):
        s = _solver(golden_sd)
        s.two_streams = two_streams
        np.random.seed(3)
        g = CooperativeStepGraph(s, *cfgs, replay=replay) if use_graph else None
        losses, per_step = [], 0
        for _ in range(4):
            n0 = _launches()
            l = g(clean, label, noisy) if use_graph else s.cooperative_step(clean, label, noisy, *cfgs)
            losses.append(_losses(l))
            per_step = _launches() - n0                   # (of the last step: no plan compilation, no queue probe)
        after4 = (_state(s), np.random.rand())
        pred = s.predict(noisy).cpu()
        extra = _losses(s.cooperative_step(clean, label, noisy, *cfgs))
        res.append(dict(losses=losses, after4=after4, pred=pred, extra=extra, after5=(_state(s), np.random.rand()), launches=per_step))
        if use_graph:
            assert g.replays == 4 and len(g.entries) == 1
            if replay == "segments":
                d = next(iter(g.entries.values())).segments.describe()
                floor = res[0]["launches"]
                print(f"bf16 segment graph: {d['nodes']} nodes, {d['segments']} segments, {d['chains']} chains; eager step: {floor} launches")
                assert floor > 0 and d["chains"] == (2 if two_streams else 1) and d["segments"] >= d["chains"] and d["nodes"] >= floor, (d, floor)
                assert (d["events"] > 0) == two_streams, d
                if two_streams:
                    assert d["queue_probe"] and all(q["overlap"] for q in d["queue_probe"]), d
    e, r = res
    bad = [f"losses of step {i + 1}" for i, (a, b) in enumerate(zip(e["losses"], r["losses"])) if not torch.equal(a, b)]
    bad += [f"after 4 steps: {x}" for x in _differs(e["after4"][0], r["after4"][0])]
    if e["after4"][1] != r["after4"][1]:
        bad.append("np.random draw after 4 steps")
    if not torch.equal(e["pred"], r["pred"]):
        bad.append("predict(noisy) after 4 steps")
    if not torch.equal(e["extra"], r["extra"]):
        bad.append("losses of the further eager step")
    bad += [f"after the further eager step: {x}" for x in _differs(e["after5"][0], r["after5"][0])]
    if e["after5"][1] != r["after5"][1]:
        bad.append("np.random draw after the further eager step")
    assert not bad, "not bit-identical: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------- 2. the remaining graph properties
def test_bf16_graph_capture_does_not_advance_training_state(golden_sd):
    """Warm-up + capture of the bf16 step leave weights, BatchNorm buffers, Adam state and the three host RNG streams untouched; eager
    calls mixed with replays keep working."""
    clean, label, noisy = _batch(2, 64, 64, seed=6)
    s = _solver(golden_sd)
    s.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)              # one eager step first: non-trivial Adam state
    before = _state(s)
    g = CooperativeStepGraph(s, CH_MSE, SP_CE)
    random.seed(1); np.random.seed(1); torch.manual_seed(1)             # noqa: E702
    probe = (random.random(), np.random.rand(), float(torch.rand(1)))
    random.seed(1); np.random.seed(1); torch.manual_seed(1)             # noqa: E702
    g.static_in = (clean, label, noisy)
    e = g._capture(g._draw_schemes())
    _same(before, _state(s))
    assert probe == (random.random(), np.random.rand(), float(torch.rand(1)))
    g.entries[(CH_MSE["mask_type"], SP_CE["mask_type"])] = e
    ref = _solver(golden_sd)
    ref.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)
    for _ in range(2):
        g(clean, label, noisy)
        ref.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)
    assert torch.equal(s.predict(noisy), ref.predict(noisy))           # eager inference after replays sees the re-packed bf16 weights
    la, lb = s.cooperative_step(clean, label, noisy, CH_MSE, SP_CE), ref.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)
    assert all(torch.equal(u.detach(), v.detach()) for u, v in zip(la, lb))
    _same(_state(ref), _state(s))


def test_bf16_replay_mode_can_be_switched_between_replays(golden_sd):
    """runtime, segments, segments, runtime replays of ONE captured bf16 graph continue one trajectory: bitwise the all-runtime run."""
    clean, label, noisy = _batch(4, 64, 64, seed=9)
    res = []
    for modes in (["runtime"] * 4, ["runtime", "segments", "segments", "runtime"]):
        s = _solver(golden_sd)
        g = CooperativeStepGraph(s, CH_MSE, SP_CE)
        losses = []
        for m in modes:
            g.set_replay_mode(m)
            losses.append(_losses(g(clean, label, noisy)))
        res.append((losses, _state(s)))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b), (a, b)
    _same(res[0][1], res[1][1])


def test_bf16_eager_steps_between_replays_keep_the_adam_count(golden_sd):
    """graph, eager, graph, graph == four eager bf16 steps, bit for bit: the device-side Adam step counter is re-seeded when the
    optimizers were stepped outside the graph object (a counter left at 1 gives the third step the bias correction of the second)."""
    clean, label, noisy = _batch(2, 64, 64, seed=6)
    ref = _solver(golden_sd)
    want = [_losses(ref.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)) for _ in range(4)]
    s = _solver(golden_sd)
    g = CooperativeStepGraph(s, CH_MSE, SP_CE)
    got = [_losses(g(clean, label, noisy)), _losses(s.cooperative_step(clean, label, noisy, CH_MSE, SP_CE)),
           _losses(g(clean, label, noisy)), _losses(g(clean, label, noisy))]
    assert int(g.state[2]) == 4
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), (i, a, b)
    _same(_state(ref), _state(s))


def test_bf16_unsynchronised_replays_see_their_own_k(golden_sd):
    """12 bf16 replays without a host sync: every replay masks with ITS k of the seeded np.random sequence (mask zero-counts per step)."""
    clean, label, noisy = _batch(4, 64, 64, seed=5)
    s = _solver(golden_sd)
    g = CooperativeStepGraph(s, CH_MSE_RT, SP_CE_RT)
    g(clean, label, noisy)                               # capture + first replay
    torch.cuda.synchronize()
    np.random.seed(11)
    rs = np.random.RandomState(11)
    expect = [(int(128 * (rs.rand() * 0.5)), int(16 * (rs.rand() * 0.5))) for _ in range(12)]      # z is 128 x 4 x 4 at 64^2: L = 128 / 16
    del g.k_log[:]
    masks = []
    for _ in range(12):
        g(clean, label, noisy)
        masks.append((s.last_masks["image"].clone(), s.last_masks["seg"].clone()))   # stream-ordered copies, no host sync
    torch.cuda.synchronize()
    assert g.k_log == [k for pair in expect for k in pair]
    assert len(set(expect)) > 6                             # the draws do differ from step to step
    for (mi, ms), (ki, ks) in zip(masks, expect):
        assert ((mi == 0).flatten(1).sum(1) == ki).all(), (ki, (mi == 0).flatten(1).sum(1))
        assert ((ms == 0).flatten(1).sum(1) == ks).all(), (ks, (ms == 0).flatten(1).sum(1))


def test_bf16_graph_dropout_draws_a_new_pattern_every_replay(golden_sd):
    """Dropout masks under bf16 replay: a new pattern every replay (device-resident RNG state), finite losses, the device step word
    `state[2]` and the host step counts advance; the eager path continues from the replayed state."""
    clean, label, noisy = _batch(4, 64, 64, seed=7)
    s = _solver(golden_sd)
    g = CooperativeStepGraph(s, DROP_MSE, DROP_CE)
    pats = []
    for i in range(4):
        losses = g(clean, label, noisy)
        assert all(torch.isfinite(v) for v in losses)
        assert int(g.state[2]) == i + 1 and all(o.step_count == i + 1 for o in s.optimizers.values())
        pats.append((s.last_masks["image"].clone(), s.last_masks["seg"].clone()))
    for a, b in zip(pats, pats[1:]):
        assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    assert not torch.equal(pats[0][0], pats[0][1])                      # image and segmentation codes get different patterns
    frac = torch.cat([p[0].flatten() for p in pats]).mean().item()
    assert 0.4 < frac < 0.6
    s.cooperative_step(clean, label, noisy, DROP_MSE, DROP_CE)
    assert all(o.step_count == 5 for o in s.optimizers.values())


# ---------------------------------------------------------------------------------------------- 3. two chains against one
@pytest.mark.parametrize("variant", ["both", "image_only", "seg_only", "no_cfgs", "no_latent_DA", "separate_training", "targeted_C", "targeted_E"])
def test_bf16_two_stream_step_is_bitwise_identical(golden_cases, golden_sd, variant):
    """The bf16 iteration on two launch chains (one backward sweep: solver.split_backward is off in bf16) against the single chain, on the
    golden-case inputs and overrides of the fp32 test: (False, True, True), everything compared with the first run."""
    C = golden_cases[{"targeted_C": "C_step_channel_spatial", "targeted_E": "E_step_soft_random"}.get(variant, "D_step_dropout")]
    args = (dev(C["clean"]), dev(C["label"]), dev(C["noisy"]))
    outs = []
    for two in (False, True, True):
        s = _solver(golden_sd)
        assert not s.split_backward
        s.two_streams = two
        if two and s._side is None:
            s._side = torch.cuda.Stream(device=s.device)
        ov_img, ov_seg = TE._overrides(C, (C["img_cfg"], C["seg_cfg"]))
        kw = dict(img_cfg=C["img_cfg"], seg_cfg=C["seg_cfg"], image_override=ov_img, seg_override=ov_seg)
        if variant == "image_only":
            kw.update(seg_cfg=None, seg_override=None)
        elif variant == "seg_only":
            kw.update(img_cfg=None, image_override=None)
        elif variant == "no_cfgs":
            kw.update(img_cfg=None, seg_cfg=None, image_override=None, seg_override=None)
        elif variant == "no_latent_DA":
            kw.update(latent_DA=False)
        elif variant == "separate_training":
            kw.update(separate_training=True)
        losses = [_losses(s.cooperative_step(*args, **kw)) for _ in range(3 if variant.startswith("targeted") else 2)]
        outs.append((losses, _state(s)))
    for losses, state in outs[1:]:
        for a, b in zip(outs[0][0], losses):
            assert torch.equal(a, b), (a, b)
        _same(outs[0][1], state)


# ---------------------------------------------------------------------------------------------- 4. saliency-forward re-use
def _decoder_forward_launches(golden_sd, name, zshape):
    """library launches of one training-mode bf16 forward of a decoder on a code of this shape (second call: weights packed, plan compiled)"""
    net = nets.build_networks(device=DEV, state_dicts={name: golden_sd[name]}, dtype="bf16")[name]
    net.train()
    z = dev(torch.relu(torch.randn(*zshape, generator=torch.Generator().manual_seed(1)))).requires_grad_(True)
    net(z)
    torch.cuda.synchronize()
    n0 = _launches()
    net(z)
    return _launches() - n0


@pytest.mark.parametrize("two_streams", [True, False])
@pytest.mark.parametrize("case", ["C_step_channel_spatial", "E_step_soft_random"])
def test_bf16_saliency_forward_reuse_is_bitwise(golden_cases, golden_sd, case, two_streams):
    """CtlNet.reuse_pass has no dtype condition (nets.py: mode 'A', no dropout, same storage / version / weight epoch), so the bf16 plans
    take the re-use path: the saliency pass runs the data-gradient-only bf16 backward on the standard pass' stored bf16 activations.
    Three steps with and without the re-use: losses, masks, weights, BatchNorm buffers, Adam state bit for bit.  Launch saving: per step
    and per perturbed code one decoder forward less and one ctl_bn_replay_running launch more (the loss-gradient launches of the re-use
    path are no more than the loss forward + backward of the plain path); the forward's launch count is read from the bf16 decoders."""
    from cooperative_training_and_latent_space_data_augmentation_amd import model_util as MU
    C = golden_cases[case]
    args = (dev(C["clean"]), dev(C["label"]), dev(C["noisy"]))
    res = []
    for reuse in (False, True):
        MU.REUSE_SALIENCY_FORWARD = reuse
        try:
            s = _solver(golden_sd)
            s.two_streams = two_streams
            ov_img, ov_seg = TE._overrides(C, (C["img_cfg"], C["seg_cfg"]))
            n0 = _launches()
            losses = [_losses(s.cooperative_step(*args, C["img_cfg"], C["seg_cfg"], image_override=ov_img, seg_override=ov_seg)) for _ in range(3)]
            res.append((losses, _state(s), {k: v.detach().cpu().clone() for k, v in s.last_masks.items()}, _launches() - n0))
        finally:
            MU.REUSE_SALIENCY_FORWARD = True
    a, b = res
    for u, v in zip(a[0], b[0]):
        assert torch.equal(u, v), (u, v)
    _same(a[1], b[1])
    assert set(a[2]) == set(b[2]) == {"image", "seg"} and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    fwd = {name: _decoder_forward_launches(golden_sd, name, tuple(C[z].shape)) for name, z in (("image_decoder", "z_i"), ("segmentation_decoder", "z_s"))}
    saved = 3 * sum(n - 1 for n in fwd.values())
    print(f"bf16 saliency re-use: {a[3]} -> {b[3]} launches in 3 steps; decoder forwards {fwd}, expected saving >= {saved}")
    assert min(fwd.values()) > 1 and b[3] <= a[3] - saved, (a[3], b[3], fwd)


# ---------------------------------------------------------------------------------------------- 5. split graph with a gradient hook
@pytest.mark.parametrize("replay", ["runtime", "segments"])
def test_bf16_split_graph_with_a_gradient_hook(golden_sd, replay):
    """The data-parallel form in process, no extra ranks: the captured bf16 step split behind backward, a hook between the forward/backward
    graph and the Adam graph.  The hook clones every network's flat gradient.  Three runs of 3 steps: split graph + hook, eager step + the
    same hook, unsplit graph (it has no hook by construction: its gradients are read from the flat gradient buffers after the replay --
    the Adam launches read them and write weights and moments only).  Gradients of every step, losses, state and the next host draw must be
    bit-identical across the three."""
    clean, label, noisy = _batch(4, 64, 64, seed=12)
    cfgs = (CH_MSE_RT, SP_CE_RT)
    grab = lambda s: {k: m._flat.grad.detach().clone() for k, m in s.model.items()}      # noqa: E731
    res = {}
    for tag in ("eager_hook", "split_graph_hook", "unsplit_graph"):
        s = _solver(golden_sd)
        seen, losses = [], []
        hook = lambda sol: seen.append(grab(sol))                                        # noqa: E731
        np.random.seed(5)
        g = None if tag == "eager_hook" else CooperativeStepGraph(s, *cfgs, replay=replay, grad_hook=hook if tag == "split_graph_hook" else None)
        for _ in range(3):
            if g is None:
                losses.append(_losses(s.cooperative_step(clean, label, noisy, *cfgs, grad_hook=hook)))
            else:
                losses.append(_losses(g(clean, label, noisy)))
                if tag == "unsplit_graph":
                    seen.append(grab(s))
        if g is not None:
            e = next(iter(g.entries.values()))
            assert (e.adam_graph is not None) == (tag == "split_graph_hook") and g.replays == 3
        torch.cuda.synchronize()
        assert len(seen) == 3
        res[tag] = (losses, [{k: v.cpu() for k, v in gr.items()} for gr in seen], _state(s), np.random.rand())
    ref = res["eager_hook"]
    assert all(float(gr[k].abs().max()) > 0 for gr in ref[1] for k in gr)
    assert not torch.equal(ref[1][0]["image_encoder"], ref[1][1]["image_encoder"])       # the hook saw each step's own gradient
    for tag in ("split_graph_hook", "unsplit_graph"):
        got = res[tag]
        for i, (a, b) in enumerate(zip(ref[0], got[0])):
            assert torch.equal(a, b), (tag, i, a, b)
        for i, (ga, gb) in enumerate(zip(ref[1], got[1])):
            for k in ga:
                assert torch.equal(ga[k], gb[k]), f"{tag}: gradient of {k} in step {i + 1}"
        _same(ref[2], got[2])
        assert ref[3] == got[3], tag


# ---------------------------------------------------------------------------------------------- 6. optimizer tail under replay
TAIL = dict(compute_dtype="bf16", use_ema=True, lr_policy="step", lr_decay_iters=1, skip_nonfinite=True)


@pytest.fixture(scope="module")
def batch32():
    return _batch(2, 32, 32, seed=5)


@pytest.fixture(scope="module")
def tail_eager(golden_sd, batch32):
    """The eager bf16 run with the whole tail on, computed once: max_grad_norm is a third of the first step's norm (read from a probe
    step with a bound far above it), so that clipping is active."""
    probe = TO._solver(golden_sd, max_grad_norm=1e9, **TAIL)
    TO._step(probe, batch32)
    norm0 = probe.optim_report()["grad_norm"]
    assert 0 < norm0 < 1e9
    return norm0 / 3, _tail_run(golden_sd, batch32, norm0 / 3, None)


def _tail_run(golden_sd, batch, max_norm, replay):
    s = TO._solver(golden_sd, max_grad_norm=max_norm, **TAIL)
    g = CooperativeStepGraph(s, CH_MSE, SP_CE, replay=replay) if replay else None
    steps, lrs = [], []
    for _ in range(4):
        losses = _losses(TO._step(s, batch, g))
        steps.append((losses, _state(s), TO._shadows(s), s._ctrl.cpu().clone()))
        lrs.append(s.scheduler_step()["image_encoder"])
    report = s.optim_report()
    s.eval()
    swapped = {k: m._flat_data.detach().cpu().clone() for k, m in s.model.items()}
    pred = s.predict(batch[2]).cpu()
    s.train()
    return dict(steps=steps, lrs=lrs, report=report, swapped=swapped, pred=pred, live=_state(s), ema_updates=s.ema_num_updates)


@pytest.mark.parametrize("replay", ["runtime", "segments"])
def test_bf16_optimizer_tail_under_replay(golden_sd, batch32, tail_eager, replay):
    """max_grad_norm (active), EMA, a step schedule advanced between the steps and the NaN guard on a bf16 solver at 2 x 32^2: 4 replayed
    steps against 4 eager ones -- losses, weights, buffers, Adam state, EMA shadows and the device control record after EVERY step.  Then
    eval() + predict(): the shadows are swapped in and must be re-packed for the bf16 kernels (a stale pack predicts with the live
    weights); train() restores the live weights."""
    max_norm, e = tail_eager
    r = _tail_run(golden_sd, batch32, max_norm, replay)
    assert e["lrs"] == r["lrs"] and e["lrs"][:3] == [5e-5, 2.5e-5, 1.25e-5] and e["lrs"][3] < e["lrs"][2]
    assert 0.0 < float(e["steps"][0][3][_ffi.OPTIM_CLIP]) < 1.0 and e["report"]["skipped_steps"] == 0      # clipping was active, nothing skipped
    for i, (a, b) in enumerate(zip(e["steps"], r["steps"])):
        assert torch.equal(a[0], b[0]), (i, a[0], b[0])
        _same(a[1], b[1])
        assert all(torch.equal(a[2][k], b[2][k]) for k in a[2]), f"EMA shadows after step {i + 1}"
        assert torch.equal(a[3], b[3]), (i, a[3].tolist(), b[3].tolist())
    assert e["report"] == r["report"] and e["ema_updates"] == r["ema_updates"] == 4
    for k in e["swapped"]:
        assert torch.equal(e["swapped"][k], e["steps"][3][2][k]) and torch.equal(r["swapped"][k], e["swapped"][k]), k      # eval() holds the shadows
        assert not torch.equal(e["swapped"][k], e["live"][0][k]), k
    assert torch.equal(e["pred"], r["pred"])
    live = _solver(golden_sd)                                              # a bf16 solver holding the LIVE weights predicts something else
    for k, m in live.model.items():
        m._flat_data.copy_(e["live"][0][k])
        m._bflat.copy_(e["live"][1][k][0])
        m._nbt.copy_(e["live"][1][k][1])
        m.weights_changed()
    assert not torch.equal(e["pred"], live.predict(batch32[2]).cpu())
    _same(e["live"], r["live"])
    _same(e["live"], e["steps"][3][1])


# ---------------------------------------------------------------------------------------------- 7. whole volume against chunks
def test_bf16_whole_volume_pass_is_bitwise_the_chunked_loop(golden_sd):
    """bf16 `predict` with eval-mode BatchNorm: slices are independent, so a 12 x 64^2 volume as ONE pass gives exactly its chunks of 5
    (5 + 5 + 2: a ragged tail) -- logits bit for bit, and the uint8 labels of predict_volume's literal loop, default call and whole-volume
    call, for n_iter 1 and 2."""
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    s = _solver(golden_sd)
    s.train()
    with torch.no_grad():                                   # non-trivial running statistics
        for i in range(2):
            c_, l_, n_ = O.synthetic_batch(2, 64, 64, seed=20 + i, structured=True)
            s.standard_training(dev(c_), dev(l_), dev(n_))
    assert all(int(m._nbt.max()) > 0 for m in s.model.values())
    vol = dev(torch.rand(12, 1, 64, 64, generator=torch.Generator().manual_seed(9)))
    for n_iter in (1, 2):
        whole = s.predict(vol, n_iter=n_iter)
        parts = torch.cat([s.predict(vol[lo:lo + 5], n_iter=n_iter) for lo in range(0, 12, 5)], 0)
        assert whole.shape == parts.shape == (12, 4, 64, 64) and torch.equal(whole, parts)
        literal = predict_volume(s, vol, n_iter=n_iter, chunk=5, coalesce=False)
        assert torch.equal(predict_volume(s, vol, n_iter=n_iter, chunk=5), literal)
        assert torch.equal(predict_volume(s, vol, n_iter=n_iter, chunk=None), literal)
        assert literal.dtype == torch.uint8 and literal.shape == (12, 64, 64)
    assert not torch.equal(s.predict(vol, n_iter=1), s.predict(vol, n_iter=2))


# ---------------------------------------------------------------------------------------------- 8. checkpoint resume
def test_bf16_checkpoint_resume(golden_cases, golden_sd, tmp_path):
    """Two bf16 steps, snapshot, a fresh bf16 solver loads it: the third step of both is bit-identical (losses, weights, buffers, Adam
    state) -- the loaded master weights reach the packed bf16 weights.  The same file loads into an fp32 solver (the master weights are fp32
    in both) and gives it the same weights, buffers and Adam state."""
    C = golden_cases["D_step_dropout"]
    ov = TE._overrides(C, (C["img_cfg"], C["seg_cfg"]))
    args = (dev(C["clean"]), dev(C["label"]), dev(C["noisy"]), C["img_cfg"], C["seg_cfg"])
    a = _solver(golden_sd)
    for _ in range(2):
        a.cooperative_step(*args, image_override=ov[0], seg_override=ov[1])
    snap = a.save_snapshots(str(tmp_path), epoch=2)
    saved = _state(a)
    c = _solver(golden_sd)
    assert c.load_snapshots(snap) == 2
    _same(saved, _state(c))
    f = _graph_solver(golden_sd)
    assert f.compute_dtype == "fp32" and f.load_snapshots(snap) == 2
    _same(saved, _state(f))
    la = a.cooperative_step(*args, image_override=ov[0], seg_override=ov[1])
    lc = c.cooperative_step(*args, image_override=ov[0], seg_override=ov[1])
    assert torch.equal(_losses(la), _losses(lc))
    _same(_state(a), _state(c))
    assert all(torch.isfinite(v) for v in f.cooperative_step(*args, image_override=ov[0], seg_override=ov[1]))      # ... and trains on in fp32


# ---------------------------------------------------------------------------------------------- 9. grouped passes (not bitwise)
@pytest.mark.parametrize("mode", ["A", "B"])
@pytest.mark.parametrize("name,n", [("shape_encoder", 3), ("shape_decoder", 2), ("image_encoder", 4), ("segmentation_decoder", 5)])
def test_bf16_grouped_pass_vs_rounding_point_oracle_run_twice(name, n, mode, golden_sd):
    """One bf16 pass over two stacked batches with BatchNorm groups (groups = 2) against the rounding-point oracle run as the two passes one
    after the other -- never against the engine itself.  The statistics partials of a grouped pass are summed in another order, so nothing
    here is bitwise.  Bounds, all the project's own: outputs 2e-2 max / 3e-3 mean of max|ref| per pass and running statistics 5e-3
    (tests/test_bf16_engine_gpu.py::test_bf16_network_forward_vs_rounding_point_oracle); num_batches_tracked exactly 2 (mode A) / 0 (mode B);
    input gradients of both groups and the SUMMED parameter gradients a <= 2 * max(own fp64-vs-fp32 distance, median) + 2 * 2^-8 per tensor
    (tests/test_bf16_backward_gpu.py::test_bf16_network_backward_vs_oracle_with_noise_yardstick)."""
    from cooperative_training_and_latent_space_data_augmentation_amd.autograd import net_apply
    c, h, w = TB.NET_INPUT[name]
    g = torch.Generator().manual_seed(11)
    if "decoder" in name:
        xs = [torch.relu(torch.randn(n, c, h, w, generator=g)), 1.3 * torch.relu(torch.randn(n, c, h, w, generator=g) + 0.2)]
    else:
        xs = [torch.rand(n, c, h, w, generator=g), torch.rand(n, c, h, w, generator=g) * 1.7 - 0.2]
    hnet = nets.build_networks(device=DEV, state_dicts={name: golden_sd[name]}, dtype="bf16")[name]
    hnet.train()
    xh = [dev(x).requires_grad_(True) for x in xs]
    if mode == "B":
        with _disable_tracking_bn_stats(hnet):
            yh = net_apply(hnet, torch.cat(xh, 0), groups=2)
    else:
        yh = net_apply(hnet, torch.cat(xh, 0), groups=2)
    yh = [tuple(o[:n] for o in yh), tuple(o[n:] for o in yh)]
    gg = torch.Generator().manual_seed(5)
    douts = [[torch.randn(o.shape, generator=gg) for o in oo] for oo in yh]
    torch.autograd.backward([o for oo in yh for o in oo], [dev(d) for dd in douts for d in dd])
    torch.cuda.synchronize()
    res = {}
    for dt in (torch.float32, torch.float64):            # the rounding-point computation in two arithmetics: their distance = the noise floor
        onet = O.build_networks(init=False)[name]
        onet.load_state_dict(golden_sd[name])
        onet = onet.to(dt)
        onet.train()
        passes = []
        for x, dd in zip(xs, douts):                     # two consecutive passes: running statistics updated in call order
            if mode == "B":
                with O.bn_no_track(onet):
                    outs, rec = P.net_forward(onet, x.to(dt))
                    passes.append((outs,) + P.net_backward(onet, rec, [d.to(dt) for d in dd]))
            else:
                outs, rec = P.net_forward(onet, x.to(dt))
                passes.append((outs,) + P.net_backward(onet, rec, [d.to(dt) for d in dd]))
        summed = {k: passes[0][2][k] + passes[1][2][k] for k in passes[0][2]}
        res[dt] = (passes, summed, {k: v.clone() for k, v in onet.named_buffers()})
    (p32, g32, b32), (p64, g64, _) = res[torch.float32], res[torch.float64]
    errs, means = [], []
    for grp in range(2):
        for a, b in zip(yh[grp], p32[grp][0]):
            assert a.dtype == torch.float32 and a.shape == b.shape
            errs.append(TB.rel_err(a, b))
            means.append(float((a.detach().cpu().double() - b.double()).abs().mean() / b.double().abs().max()))
    hb = dict(hnet.named_buffers())
    berr = max(float((hb[k].cpu().double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-6))
               for k, b in b32.items() if b.dtype.is_floating_point)
    rows = [(f"dx of group {grp}", TBB.rel(xh[grp].grad, p32[grp][1]), TBB.rel(p64[grp][1], p32[grp][1])) for grp in range(2)]
    hp = dict(hnet.named_parameters())
    for k, gr in g32.items():
        if not k.endswith(TBB.DEAD):
            rows.append((k, TBB.rel(hp[k].grad, gr), TBB.rel(g64[k], gr)))
    med = float(np.median([r[2] for r in rows]))
    print(f"bf16 grouped {name} mode {mode}: output max err {max(errs):.2e} mean err {max(means):.2e} (of max|ref|), running statistics {berr:.2e}, "
          f"worst gradient HIP-vs-oracle {max(r[1] for r in rows):.3f}, worst oracle fp64-vs-fp32 {max(r[2] for r in rows):.3f}, median {med:.3f}")
    assert max(errs) <= 2e-2 and max(means) <= 3e-3, (name, mode, errs, means)
    assert berr <= 5e-3, (name, mode, berr)
    nbt = [k for k in hb if k.endswith("num_batches_tracked")]
    assert nbt and all(int(hb[k]) == (2 if mode == "A" else 0) for k in nbt)
    bad = [(k, f"{a:.3f}", f"{b:.3f}") for k, a, b in rows if not a <= 2.0 * max(b, med) + 2 * TBB.STEP]
    assert not bad, bad[:8]
    if mode == "B":
        for k, p in hp.items():
            if k not in g32:
                assert float(p.grad.abs().max()) == 0.0, k                 # gamma / beta frozen in mode B


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped_stn", "one_pass_per_call"])
def test_bf16_step_with_and_without_grouped_stn_passes_vs_oracle(golden_sd, grouped):
    """The default bf16 step runs its STN passes grouped (solver.group_stn_passes, groups = 2); off = one pass per reference call.  Each form
    against the forward-only rounding-point oracle that is given that run's mask selection, with the bounds of
    tests/test_bf16_engine_gpu.py::test_bf16_cooperative_step_vs_rounding_point_oracle: 1e-2 on the first three losses, 6e-2 on all."""
    clean, label, noisy = O.synthetic_batch(4, 64, 64, seed=4, structured=True)
    s = _solver(golden_sd)
    s.group_stn_passes = grouped
    n0 = _launches()
    losses = s.cooperative_step(dev(clean), dev(label), dev(noisy), CH_MSE, SP_CE, do_optim=False)
    got = _losses(losses).double()
    n1 = _launches()
    o = O.OracleSolver(state_dicts=golden_sd)
    with O.bf16_rounding_points():
        ref = o.cooperative_step(clean, label, noisy, CH_MSE, SP_CE, do_optim=False,
                                 image_override={"mask": s.last_masks["image"].cpu()}, seg_override={"mask": s.last_masks["seg"].cpu()})
    err = (got - torch.tensor(ref, dtype=torch.float64)).abs()
    print(f"bf16 step, group_stn_passes={grouped}: {n1 - n0} launches, losses {got.tolist()}, rounding-point oracle {list(ref)}, |diff| {err.tolist()}")
    assert float(err[:3].max()) <= 1e-2 and float(err.max()) <= 6e-2, (got, ref)
    assert ((s.last_masks["image"] == 0).flatten(1).sum(1) == 64).all() and ((s.last_masks["seg"] == 0).flatten(1).sum(1) == 8).all()
