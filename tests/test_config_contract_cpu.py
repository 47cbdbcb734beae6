"""The supported set of (image_ch, num_classes, reduce_factor, dtype) is a contract, decided at construction (nets.check_config): a
configuration the kernels cannot serve is a ValueError from nets.build_networks and from the solver's constructor, before any storage is
allocated; every other one compiles every plan the engine can ask for, and its networks are the oracle's networks (same parameters, same
state-dict keys, same output shapes).  Plans are compiled on device="cpu"; no kernel runs here (tests/test_config_engine_gpu.py does that)."""
import itertools

import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, init, nets, solver
from oracle import ref_cpu as O

GRID = list(itertools.product([1, 3, 4], [1, 2, 3, 4, 8, 12, 16, 20], [1, 2, 4, 8, 16], ["fp32", "bf16"]))
SIZES = [(2, 48, 64), (3, 80, 112)]                          # encoder inputs; the latents are 16 x smaller


def the_rules(image_ch, num_classes, reduce_factor, dtype):
    """the library's rules written out once more, independently of nets.check_config: ctl_conv_pick_cfg (cin 1 / 4 / 8 / 12 / 16k, cout 1 / 4k:
    a tensor is both), MAXC = 16 classes in the label-space kernels, whole 16-channel tiles for a bf16-stored tensor, CTL_PRO_MAX = 256
    BatchNorm coefficients staged by the conv that applies them (the widest BatchNorm is 512 // reduce_factor wide).  -> the offending parameter"""
    both = lambda c: c in (1, 4, 8, 12) or (c >= 16 and c % 16 == 0)
    if not both(image_ch):
        return "image_ch"
    if not both(num_classes) or num_classes > 16:
        return "num_classes"
    widths = [64 // reduce_factor, 128 // reduce_factor, 256 // reduce_factor, 512 // reduce_factor]
    if not all(both(c) and (dtype == "fp32" or c % 16 == 0) for c in widths) or max(widths) > 256:
        return "reduce_factor"
    return None


def compile_forward(net, n, h, w, mode, groups=1):
    return net._compile_forward(n, h, w, mode, groups=groups)


def compile_backward(net, fwd, groups, mask, need_dx):
    assert fwd.groups == groups                    # a backward plan has the BatchNorm groups of its forward pass
    return net._compile_backward(fwd, "A", mask, need_dx, True, True)


def check_records(plan, dtype):
    """what the conv records of a plan may ask of the library at a width off the 16-grid"""
    ops, k, entries = plan.ops, 0, 0
    while k < len(ops):
        kind = int(ops[k]["kind"])
        if kind == _ffi.OP_WGRAD_GROUP:
            for m in ops[k + 1:k + 1 + _ffi.op_field(ops[k], "members")]:
                d = _ffi.op_field(m, "conv")
                assert int(m["kind"]) == _ffi.OP_WGRAD
                assert d["cin"] % 16 == 0 and d["cout"] % 16 == 0, f"a {d['cin']} -> {d['cout']} weight gradient rides in a grouped launch"
        if kind in (_ffi.OP_CONV, _ffi.OP_WGRAD):
            d = _ffi.op_field(ops[k], "conv")
            cin, cout, dt = int(d["cin"]), int(d["cout"]), int(d["dt"])
            if dtype == "fp32":
                assert not dt & ~_ffi.DT_X3
                if cin % 16 != 0:
                    assert dt == 0, f"{cin} -> {cout}: a padded cin chunk stays on the fp32 pipe"
                if dt & _ffi.DT_X3:
                    assert cout % 16 == 0 or (kind == _ffi.OP_CONV and cout in (4, 8, 12)), f"X3 at {cin} -> {cout}"
            else:
                assert not (dt & _ffi.DT_X16) or cin % 16 == 0
                assert not (dt & (_ffi.DT_Y16 | _ffi.DT_RES16)) or cout % 16 == 0
            if kind == _ffi.OP_CONV and int(d["pro_affine"]) == 2:
                assert cin % 16 == 0
            if kind == _ffi.OP_CONV and int(d["epi_flags"]) & _ffi.EPI_TAILBWD:
                assert cout % 16 == 0, f"{cin} -> {cout}: CTL_EPI_TAILBWD is refused at launch for a partial cout tile"
            if kind == _ffi.OP_CONV and dtype == "bf16" and int(d["epi_flags"]) & _ffi.EPI_BNBWD:
                assert cin % 16 == 0 and cout % 16 == 0
            if int(d["pro_affine"]) == 1:
                entries = max(entries, max(int(d["groups"]), 1) * cin)
        k += 1
    assert entries == plan.pro_entries, "Plan.pro_entries is the largest groups * cin of a launch with the activation prologue"
    return entries


def fits(net, plan, entries, groups):
    """one pass (groups = 1) always fits the kernels' 256-entry prologue table; a grouped pass that does not is refused as a whole by
    run_forward / run_backward before its first launch (the encoders at reduce_factor 2: 2 x 256), never half-way through a plan"""
    assert groups > 1 or entries <= 256
    if entries > 256:
        with pytest.raises(_ffi.CtlError, match=f"groups \\* cin = {entries}"):
            net._check_prologue_tables(plan)
    else:
        net._check_prologue_tables(plan)


@pytest.mark.parametrize("image_ch,num_classes,reduce_factor,dtype", GRID, ids=["-".join(map(str, g)) for g in GRID])
def test_every_grid_point_is_refused_at_construction_or_compiles_every_plan(image_ch, num_classes, reduce_factor, dtype):
    cfg = (image_ch, num_classes, reduce_factor)
    bad = the_rules(*cfg, dtype)
    if bad is not None:
        with pytest.raises(ValueError) as e:
            nets.build_networks(*cfg, device="cpu", dtype=dtype)
        value = dict(image_ch=image_ch, num_classes=num_classes, reduce_factor=reduce_factor)[bad]
        assert f"{bad}={value}" in str(e.value) and ("accepted" in str(e.value) or "1, 4, 8, 12" in str(e.value)), str(e.value)
        with pytest.raises(ValueError):
            nets.check_config(*cfg, dtype)
        if reduce_factor == 4:                                  # (the solver builds reduce_factor 4)
            with pytest.raises(ValueError):
                solver.AdvancedTripletReconSegmentationModel(image_ch=image_ch, num_classes=num_classes, compute_dtype=dtype)
        print(f"{cfg + (dtype,)}: ValueError ({bad})")
        return
    torch.manual_seed(0)
    sd = init.reference_init_state_dicts(*cfg)
    model = nets.build_networks(*cfg, device="cpu", state_dicts=sd, dtype=dtype)      # a CtlError anywhere below fails the test
    oracle = O.build_networks(*cfg, init=False)
    z = 512 // reduce_factor
    for name, net in model.items():
        ref = oracle[name]
        ref.load_state_dict(sd[name], strict=True)
        ref.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()}, strict=True)      # the round trip
        assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters()), name
        enc = name.endswith("encoder")
        for n, h, w in SIZES:
            if not enc:
                h, w = h // 16, w // 16
            cin = {"image_encoder": image_ch, "shape_encoder": num_classes}.get(name, z)
            with torch.no_grad():
                out = ref.eval()(torch.zeros(n, cin, h, w))
            want = [(o.shape[0], o.shape[2], o.shape[3], o.shape[1]) for o in (out if isinstance(out, (tuple, list)) else (out,))]
            for groups in ((1, 2) if n % 2 == 0 else (1,)):
                for mode in "ABC":
                    fwd = compile_forward(net, n, h, w, mode, groups)
                    assert [tuple(s) for s in fwd.out_shapes] == want, (name, mode, fwd.out_shapes, want)
                    fits(net, fwd, check_records(fwd, dtype), groups)
                fwd = compile_forward(net, n, h, w, "A", groups)
                bwd = compile_backward(net, fwd, groups, (True,) * len(want), name != "image_encoder")
                fits(net, bwd, check_records(bwd, dtype), groups)
                if reduce_factor == 8 and groups == 1:
                    members = sum(_ffi.op_field(o, "members") for o in bwd.ops if int(o["kind"]) == _ffi.OP_WGRAD_GROUP)
                    print(f"  {name} {n}x{h}x{w}: {members} grouped weight gradients")
    print(f"{cfg + (dtype,)}: compiled")


def test_the_check_names_parameter_value_and_accepted_values():
    for kw, words in [(dict(image_ch=3), ["image_ch=3", "1, 4, 8, 12"]), (dict(num_classes=2), ["num_classes=2", "[1, 4, 8, 12, 16]"]),
                      (dict(num_classes=20), ["num_classes=20", "at most 16"]), (dict(reduce_factor=8, dtype="bf16"), ["reduce_factor=8", "[2, 4]", "bf16"]),
                      (dict(reduce_factor=3), ["reduce_factor=3", "[2, 4, 8, 16]"]), (dict(reduce_factor=1), ["reduce_factor=1", "[2, 4, 8, 16]", "256"]), (dict(reduce_factor=0), ["reduce_factor=0"]),
                      (dict(dtype="fp16"), ["fp16", "bf16"])]:
        with pytest.raises(ValueError) as e:
            nets.check_config(**kw)
        assert all(w in str(e.value) for w in words), (kw, str(e.value))
    nets.check_config()                                          # the shipped model


def test_refusal_comes_before_any_storage(monkeypatch):
    """nothing is drawn, constructed or allocated for a refused configuration"""
    def boom(*a, **k):
        raise AssertionError("storage was touched before the configuration check")
    monkeypatch.setattr(init, "reference_init_state_dicts", boom)
    monkeypatch.setattr(nets.CtlNet, "__init__", boom)
    for cfg, dtype in [((3, 4, 4), "fp32"), ((1, 2, 4), "fp32"), ((1, 4, 8), "bf16")]:
        with pytest.raises(ValueError):
            nets.build_networks(*cfg, device="cpu", dtype=dtype)
    monkeypatch.setattr(solver, "build_networks", boom)
    with pytest.raises(ValueError):
        solver.AdvancedTripletReconSegmentationModel(num_classes=3)
