"""Network parity against fp64 at the shapes where the conv / weight-gradient launches of a compiled plan switch their kernel form
(fp32 engine, the default X3 arithmetic).  The ladder, the picker arithmetic behind every rung, the tolerance rule and the measured
figures are in tests/form_ladder.py; the comparison itself is tested without a GPU in tests/test_form_ladder_cpu.py.

Four kinds of test:
  test_rung_parity_*            three evaluations per rung (fp64 oracle, the same oracle in fp32 on the CPU, the HIP network) on the
                                inputs and weights of tests/test_engine_gpu.make_pair: outputs, dx, every parameter gradient, buffers
  test_rung_takes_its_forms     the ids first reached at every rung are the ones form_ladder.RUNG_NEW records
  test_workload_forms_are_on_the_ladder   every conv-family id of the bs16 x 256^2 step (dropout and targeted masks), of `predict` at
                                10 x 192^2 and of the 40-slice whole-volume pass is taken by some rung (UNCOVERED: the exceptions)
  test_plan_branches_without_an_id        fused sum-pool, statistics rows of a multi-round persistent grid, split counts, grouped
                                launches: asserted through the library's host queries on the layer's descriptor and on the plan"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import form_ladder as L  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, nets  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd.model_util import _disable_tracking_bn_stats  # noqa: E402
from test_engine_gpu import DEV, dev, is_dead_bias, make_pair  # noqa: E402

# workload ids no rung takes: id -> (reason, kernel-level test that covers the form).  At most four; empty unless the picker arithmetic
# shows the form cannot be reached below the workload's own shape.
UNCOVERED = {}

_IDS = {}          # (network, "train" | "eval", rung) -> conv-family ids of the HIP run (filled by the parity tests, or on demand)
_PLANS = {}        # (network, rung) -> (forward plan, backward plan) of the mode-A run


def _tuple(y):
    return y if isinstance(y, tuple) else (y,)


def _hip_train(name, hnet, x, douts, mode, rung):
    """forward + backward of the HIP network; mode A: under the census"""
    xh = dev(x).requires_grad_(True)
    out = {}

    def run():
        if mode == "B":
            with _disable_tracking_bn_stats(hnet):
                y = _tuple(hnet(xh))
        else:
            y = _tuple(hnet(xh))
        out["y"] = y
        torch.autograd.backward(y, [torch.ones_like(t) for t in y] if douts is None else [dev(d) for d in douts])
    if mode == "A":
        hnet._plans.clear()
        _IDS[(name, "train", rung)] = L.census(run)
        _PLANS[(name, rung)] = {k[0]: p for k, p in hnet._plans.items() if k[0] in ("f", "b")}
    else:
        run()
    return out["y"], xh.grad


def ladder_ids(name, kind, rung, golden_sd):
    key = (name, kind, rung)
    if key not in _IDS:
        hnet = nets.build_networks(device=DEV, state_dicts={name: golden_sd[name]})[name]
        x, g = L.rung_input(name, rung)
        if kind == "train":
            hnet.train()
            _hip_train(name, hnet, x, None, "A", rung)
        else:
            hnet.eval()
            with torch.no_grad():
                _IDS[key] = L.census(lambda: hnet(dev(x)))
    return _IDS[key]


def _report(figures, bad, title):
    for what, cls, m, e_cpu, e_hip in figures:
        print(f"FIGURE {title} | {what} | {cls} | {m} | e_cpu {e_cpu:.3e} | e_hip {e_hip:.3e} | ratio {e_hip / max(e_cpu, 1e-300):.2f}")
    assert not bad, f"{title}: {len(bad)} tensors outside max(3 x e_cpu, floor):\n" + "\n".join(bad[:12])


def _train_rung(name, rung, mode, golden_sd):
    onet, hnet = make_pair(name, golden_sd)
    o64 = copy.deepcopy(onet).double()
    for m in (onet, o64, hnet):
        m.train()
    x, g = L.rung_input(name, rung)
    res = {}
    douts = None
    for tag, net, xin in (("f64", o64, x.double()), ("f32", onet, x.clone())):
        xin.requires_grad_(True)
        if mode == "B":
            with O.bn_no_track(net):
                y = _tuple(net(xin))
        else:
            y = _tuple(net(xin))
        if douts is None:
            douts = [torch.randn(t.shape, generator=g) for t in y]
        torch.autograd.backward(y, [d.to(t.dtype) for d, t in zip(douts, y)])
        res[tag] = (y, xin.grad, dict(net.named_parameters()), dict(net.named_buffers()))
    yh, dxh = _hip_train(name, hnet, x, douts, mode, rung)
    (y64, dx64, p64, b64), (y32, dx32, p32, b32) = res["f64"], res["f32"]
    hp, hb = dict(hnet.named_parameters()), dict(hnet.named_buffers())
    figures, bad = [], []
    for i, (a, b, c) in enumerate(zip(yh, y32, y64)):
        bad += L.judge("output", f"output {i}", a, b, c, figures)
    bad += L.judge("dx", "dx", dxh, dx32, dx64, figures)
    for n, p in p64.items():
        if mode == "B" and p.grad is None:                 # gamma / beta are frozen in mode B
            assert float(hp[n].grad.abs().max()) == 0.0, n
            continue
        if is_dead_bias(n):                                # true gradient exactly 0: today's rule (tests/test_engine_gpu.py)
            wn = float(p64[n[:-4] + "weight"].grad.norm())
            assert float(hp[n].grad.abs().max()) <= 1e-3 * wn + 1e-4, n
            continue
        bad += L.judge(L.grad_class(p.grad), f"grad {n}", hp[n].grad, p32[n].grad, p.grad, figures)
    for n, b in b64.items():
        if n.endswith("num_batches_tracked"):
            assert int(hb[n]) == int(b) == (1 if mode == "A" else 0), n
            continue
        bad += L.judge("buffer", f"buffer {n}", hb[n], b32[n], b, figures)
    _report(figures, bad, f"{name} {L.rung_id(rung)} mode {mode}")


def _params(table):
    return [pytest.param(name, rung, id=f"{name}-{L.rung_id(rung)}") for name in L.NETS for rung in table.get(name, [])]


@pytest.mark.parametrize("name,rung", _params(L.LADDER))
def test_rung_parity_training_mode_a(name, rung, golden_sd):
    _train_rung(name, rung, "A", golden_sd)


@pytest.mark.parametrize("name,rung", _params({k: [v] for k, v in L.MODE_B_RUNG.items()}))
def test_rung_parity_training_mode_b(name, rung, golden_sd):
    """BatchNorm without tracking (batch statistics, frozen affine pair, buffers untouched) on one large rung per network"""
    _train_rung(name, rung, "B", golden_sd)


@pytest.mark.parametrize("name,rung", _params(L.EVAL_LADDER))
def test_rung_parity_inference(name, rung, golden_sd):
    """forward with eval-mode BatchNorm on running statistics that one training pass has moved; all three networks hold the same
    weights and buffers (the oracle's)"""
    onet = O.build_networks(init=False)[name]
    onet.load_state_dict(golden_sd[name])
    onet.train()
    warm, _ = L.rung_input(name, (2, 32, 32) if "encoder" in name else (2, 2, 2), seed=5)
    with torch.no_grad():
        onet(warm * 1.5)
    onet.eval()
    sd = {k: v.clone() for k, v in onet.state_dict().items()}
    hnet = nets.build_networks(device=DEV, state_dicts={name: sd})[name]
    hnet.eval()
    o64 = copy.deepcopy(onet).double()
    x, _ = L.rung_input(name, rung)
    with torch.no_grad():
        y64, y32 = _tuple(o64(x.double())), _tuple(onet(x))
        out = {}
        _IDS[(name, "eval", rung)] = L.census(lambda: out.update(y=_tuple(hnet(dev(x)))))
    figures, bad = [], []
    for i, (a, b, c) in enumerate(zip(out["y"], y32, y64)):
        bad += L.judge("output", f"output {i}", a, b, c, figures)
    _report(figures, bad, f"{name} {L.rung_id(rung)} eval")


@pytest.mark.parametrize("name", L.NETS)
def test_rung_takes_its_forms(name, golden_sd):
    """Walking up the ladder, the ids a rung adds to those of the smaller rungs are the recorded ones: a heuristic change that moves a
    layer to another form shows here by id."""
    seen, diff = set(), []
    for kind, table in (("train", L.LADDER), ("eval", L.EVAL_LADDER)):
        for rung in table.get(name, []):
            ids = ladder_ids(name, kind, rung, golden_sd)
            new, want = ids - seen, set(L.RUNG_NEW.get(name, {}).get(kind, {}).get(L.rung_id(rung), []))
            print(f"FORMS {name} {kind} {L.rung_id(rung)}: {len(ids)} ids, new: {sorted(new)}")
            if new != want:
                diff.append(f"{kind} {L.rung_id(rung)}: no longer first reached here {sorted(want - new)}, newly first reached here {sorted(new - want)}")
            seen |= ids
    assert not diff, f"{name}: the forms of the ladder moved\n" + "\n".join(diff)
    if "encoder" in name:       # both sides of the stride-2 data-gradient branch (nets.py, _emit_block_bwd): four phase problems / zero-insert
        assert any(i.startswith("conv_igemm_x3<ks2,s1,in0") for i in seen) and any(i.startswith("conv_igemm_x3<ks3,s1,in2") for i in seen), sorted(seen)


def test_workload_forms_are_on_the_ladder(golden_sd):
    import bench
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import predict_volume
    s = AdvancedTripletReconSegmentationModel(use_gpu=True)
    clean, label, noisy, _ = bench.synthetic(16, 256, 256, 7, torch.device(DEV))
    work = {}
    for masks, cfg in (("dropout", (bench.DROP_IMG, bench.DROP_SEG)), ("targeted", (bench.TGT_IMG, bench.TGT_SEG))):
        work[f"step, {masks} masks"] = L.census(lambda: [s.cooperative_step(clean, label, noisy, *cfg) for _ in range(2)])
    vol = dev(torch.rand(40, 1, 192, 192, generator=torch.Generator().manual_seed(9)))
    work["predict 10 x 192^2"] = L.census(lambda: [s.predict(vol[:10], n_iter=k) for k in (1, 2)])
    work["whole volume 40 x 192^2"] = L.census(lambda: [predict_volume(s, vol, n_iter=k, chunk=None) for k in (1, 2)])
    del s
    ladder = set()
    for kind, table in (("train", L.LADDER), ("eval", L.EVAL_LADDER)):
        for name, rungs in table.items():
            for rung in rungs:
                ladder |= ladder_ids(name, kind, rung, golden_sd)
    assert len(UNCOVERED) <= 4
    missing = {w: sorted(ids - ladder - set(UNCOVERED)) for w, ids in work.items()}
    for w, ids in work.items():
        print(f"WORKLOAD {w}: {len(ids)} ids, {len(ids - ladder)} not on the ladder")
        assert len(ids) >= 10, (w, ids)
    assert not any(missing.values()), f"forms the workloads use that no rung compares with fp64: {missing}"
    stale = sorted(i for i in UNCOVERED if i in ladder or not any(i in ids for ids in work.values()))
    assert not stale, f"UNCOVERED lists ids that a rung takes or no workload uses: {stale}"


def _plan_ops(name, rung, which, golden_sd):
    ladder_ids(name, "train", rung, golden_sd)
    return _PLANS[(name, rung)][which].ops


def test_plan_branches_without_an_id(golden_sd):
    lib, P = _ffi.lib, _ffi.desc_ptr
    S, TAIL = _ffi.EPI_STATS, _ffi.EPI_TAILBWD
    # 1. the decoder's tail 1x1 (data gradient 4 -> 16 of the last conv, CTL_EPI_TAILBWD): the epilogue writes the 2x2 sum-pool only on the
    #    8x16 / 8x32 tiles -- segmentation_decoder 3x4x3 (3 x 64 x 48: 4x16 tile) no, 1x16x16 (1 x 256 x 256: 8x16) yes
    tail = lambda n, h, w: _ffi.conv_desc(n=n, hin=h, win=w, cin=4, hout=h, wout=w, cout=16, ks=1, epi_flags=S | TAIL)
    assert lib.ctl_conv_pool_ok(P(tail(3, 64, 48))) == 0 and lib.ctl_conv_pool_ok(P(tail(1, 256, 256))) == 1
    for rung, want in (((3, 4, 3), False), ((1, 16, 16), True)):      # ... and the compiled plans follow the answer
        ops = _plan_ops("segmentation_decoder", rung, "b", golden_sd)
        hosts = [o for o in ops if int(o["kind"]) == _ffi.OP_CONV and int(_ffi.op_field(o, "conv")["ks"]) == 1 and int(_ffi.op_field(o, "conv")["cin"]) == 4]
        assert len(hosts) == 1 and (_ffi.op_field(hosts[0], "pool")[0] >= 0) == want, rung
        assert any(int(o["kind"]) == _ffi.OP_SUMPOOL2 for o in ops)      # (the lower blocks still pool in a pass of their own)
    # 2. statistics rows: image_encoder 8x256x256, 16 -> 16 @ 256^2 on the 8x32 tile = 8 * 32 * 8 = 2048 tiles on a persistent grid of fewer
    #    blocks, so every block accumulates several tiles into its row
    d = _ffi.conv_desc(n=8, hin=256, win=256, cin=16, hout=256, wout=256, cout=16, ks=3, epi_flags=S | _ffi.EPI_BIAS, dt=_ffi.DT_X3)
    rows = lib.ctl_conv_stats_blocks(P(d))
    assert 0 < rows < 8 * 32 * 8, rows
    assert "conv_igemm_x3<ks3,s1,in0,mt4,tw32,nt1>" in ladder_ids("image_encoder", "train", (8, 256, 256), golden_sd)
    d3 = _ffi.conv_desc(n=3, hin=40, win=56, cin=16, hout=40, wout=56, cout=16, ks=3, epi_flags=S | _ffi.EPI_BIAS, dt=_ffi.DT_X3)
    assert lib.ctl_conv_stats_blocks(P(d3)) == 3 * 10 * 4               # 3x40x56: one 4x16 tile per block, one round
    # 3. weight-gradient splits: 128 -> 128 3x3 at h/16 -- image_encoder 1x128x128: 8x8 is one 8x16 tile, one split; 8x256x256: 16 splits
    wg = lambda n, h: _ffi.conv_desc(n=n, hin=h, win=h, cin=128, hout=h, wout=h, cout=128, ks=3, dt=_ffi.DT_X3)
    assert lib.ctl_wgrad_splits(P(wg(1, 8))) == 1 and lib.ctl_wgrad_splits(P(wg(8, 16))) > 1
    # 4. a grouped launch of at least two members at image_encoder 8x256x256 (its seven two-tensor 3x3 weight gradients share one)
    ops = _plan_ops("image_encoder", (8, 256, 256), "b", golden_sd)
    members = [_ffi.op_field(o, "members") for o in ops if int(o["kind"]) == _ffi.OP_WGRAD_GROUP]
    assert members and max(members) >= 2, members
    assert lib.ctl_wgrad_group_class(P(wg(8, 16)), 1) == lib.ctl_wgrad_group_class(P(wg(8, 32)), 1) >= 0
    descs = np.concatenate([np.atleast_1d(wg(8, 16)), np.atleast_1d(wg(8, 32))])
    splits = np.zeros(2, dtype=np.int32)
    _ffi.check(lib.ctl_wgrad_group_plan(descs.ctypes.data, 2, splits.ctypes.data), "ctl_wgrad_group_plan")
    assert (splits >= 1).all() and splits[1] > splits[0]                # (CUs dealt in proportion to the members' pixel tiles)
    #    ... and the members' split counts in the plan are the partial-buffer sizes the reduction table holds (tests/test_host_logic.py)
    grp = [k for k, o in enumerate(ops) if int(o["kind"]) == _ffi.OP_WGRAD_GROUP]
    for k in grp:
        for m in ops[k + 1:k + 1 + _ffi.op_field(ops[k], "members")]:
            assert int(m["kind"]) == _ffi.OP_WGRAD and _ffi.op_field(m, "group_splits") >= 1
