"""Weight gradients behind guard bands: ctl_conv_wgrad_ex writes split-K partials sized by ctl_wgrad_partial_floats /
ctl_wgrad_bias_partial_floats, ctl_wgrad_reduce(_batched) scatters their sum with generic strides into the flat gradient buffer, where the
neighbours of a layer's range are other layers' gradients (nets.py: one `grad` tensor, ranges at 64-float alignment).

Every case: the partial buffers are Guarded payloads of exactly the queried size, poisoned (a split the kernel skipped reaches dW as a NaN
through the reduction); dW and db are ranges of a flat_with_gaps buffer between three foreign ranges pre-filled with known finite values,
which must come back bit for bit, with poisoned alignment gaps; results against fp64 autograd by the rule of the family's own file
(fp32 3e-4, tests/test_kernels_gpu.py; X3 errs(), tests/test_x3_gpu.py; bf16 3e-4 / 1e-3 at the same rounding points,
tests/test_bf16_gpu.py); then everything is poisoned again and the identical calls must give identical bits."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check  # noqa: E402
from oracle.guarded import Guarded, GuardedCall  # noqa: E402
from oracle.guard_conv import (DEV, FAMILIES, NARROW, OFFGRID, PC, RAGGED, SLOPE, close16, close32, dev, errs, f64, fam_dt, gen_for, group_index, leaky,  # noqa: E402
                               per_group, rb, refused)

NEIGHBOURS = (37, 129, 5)                                    # floats of the foreign ranges before, between and behind dW and db


def wgrad_ok(fam, cin, cout, ks):
    if fam == "x3":
        return ks in (2, 3) and cin % 16 == 0 and cout % 16 == 0
    return True


def run_wgrad(kw, x, dy, strides, dw_shape, accumulate=0, base=None, pro=None, dy2=None, coef=None, want_bias=True, again=True):
    """one guarded ctl_conv_wgrad_ex + ctl_wgrad_reduce: returns (dW, db) of the first run as CPU tensors"""
    d = _ffi.conv_desc(**kw)
    dp = _ffi.desc_ptr(d)
    cout = int(kw["cout"])
    nw, nb = int(lib.ctl_wgrad_partial_floats(dp)), int(lib.ctl_wgrad_bias_partial_floats(dp))
    assert int(lib.ctl_wgrad_splits(dp)) > 0 and nw > 0 and nb > 0, "the size queries refused the descriptor"
    gc = GuardedCall(DEV)
    wpart = gc.out("w_partial", nw, written=False)
    bpart = gc.out("b_partial", nb, written=False) if want_bias else None
    ndw = int(np.prod(dw_shape))
    gen = torch.Generator().manual_seed(ndw)
    foreign = [torch.randn(k, generator=gen).to(DEV) for k in NEIGHBOURS]
    based = None if base is None else (base[0].to(DEV).contiguous(), base[1].to(DEV))

    def init(f):
        for i, t in zip((0, 2, 4), foreign):
            f.range(i).copy_(t)
        if accumulate:
            f.range(1).copy_(based[0].reshape(-1))
            f.range(3).copy_(based[1])

    grad = gc.flat("grad", [NEIGHBOURS[0], ndw, NEIGHBOURS[1], cout, NEIGHBOURS[2]], written=[1, 3] if want_bias else [1], init=init)
    p = lambda t: None if t is None else t.data_ptr()

    def launch():
        check(lib.ctl_conv_wgrad_ex(dp, x.data_ptr(), p(pro[0]) if pro else None, p(pro[1]) if pro else None, dy.data_ptr(), p(dy2), p(coef), wpart.ptr,
                                    bpart.ptr if want_bias else None, ops.stream_ptr()), "ctl_conv_wgrad_ex")
        check(lib.ctl_wgrad_reduce(dp, wpart.ptr, bpart.ptr if want_bias else None, grad.range_ptr(1), *[int(s) for s in strides],
                                   grad.range_ptr(3) if want_bias else None, int(accumulate), ops.stream_ptr()), "ctl_wgrad_reduce")

    def foreign_intact():
        for i, t in zip((0, 2, 4), foreign):
            assert torch.equal(grad.range(i).view(torch.int32), t.view(torch.int32)), f"the foreign gradient range {i} next to dW / db was changed"
        if not want_bias:
            assert bool((grad.buf.bits()[grad.offsets[3]:grad.offsets[3] + cout] == 0x7FC5A5A5).all()), "db was written without a bias partial"

    gc.run(launch)
    foreign_intact()
    dw, db = grad.range(1).cpu().clone(), grad.range(3).cpu().clone()
    if again:                                                   # (False: the fp32 companion of an X3 case, which its own parameter repeats)
        gc.rerun(launch)
        foreign_intact()
    return dw, db


def oihw(dw_flat, cout, cin, ks):
    return dw_flat.view(cout, cin, ks, ks)


def judge_w(fam, got, ref, what, rel16=3e-4, got32=None):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite (a partial sum nobody wrote was reduced)"
    if fam == "fp32":
        close32(got, ref, 3e-4, what)
    elif fam == "x3":
        assert got32 is not None, f"{what}: the X3 rule needs the fp32 kernel's result on the same problem"
        errs(got, got32, ref, what)
    else:
        close16(got, ref, rel16, what)


FORMS = {    # ks, stride, up
    "3x3": (3, 1, 0), "3x3_s2": (3, 2, 0), "3x3_up2": (3, 1, 1), "1x1": (1, 1, 0), "1x1_up2": (1, 1, 1), "2x2_s2": (2, 2, 0),
}


def wgrad_cases(shapes, forms):
    return [pytest.param(form, *s, f, id=f"{form}-" + "-".join(map(str, s)) + f"-{f}") for form in forms for s in shapes for f in FAMILIES
            if wgrad_ok(f, s[1], s[2], FORMS[form][0])]


@pytest.mark.parametrize("form,n,cin,cout,h,w,fam", wgrad_cases(RAGGED + PC, list(FORMS)) + wgrad_cases(NARROW[2:4], ["3x3", "1x1", "1x1_up2"])
                         + wgrad_cases(OFFGRID, list(FORMS)))
def test_wgrad_partials_and_strided_reduce(form, n, cin, cout, h, w, fam):
    """kernel sizes 1, 2, 3; stride 2; nearest-up-sampled input; every form plain and with the activation prologue; accumulate 0 and 1
    on the plain launch (the reduction is the same kernel either way), and on the prologue launch of the 3x3 stride-1 form as well"""
    ks, stride, up = FORMS[form]
    fams = ("fp32", "x3") if fam == "x3" else (fam,)
    g = gen_for(n, cin, cout, h, w, ks, stride, up)
    hx, wx = (2 * h, 2 * w) if ks == 2 else (h, w)          # 2x2 stride 2: the input is the fine tensor
    x0 = torch.randn(n, cin, hx, wx, generator=g)
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    pad = 1 if ks == 3 else 0
    hi, wi = (2 * hx, 2 * wx) if up else (hx, wx)
    ho, wo = (hi + 2 * pad - ks) // stride + 1, (wi + 2 * pad - ks) // stride + 1
    dy0 = torch.randn(n, cout, ho, wo, generator=g)
    base = (torch.randn(cout, cin, ks, ks, generator=g), torch.randn(cout, generator=g))
    res = {}
    for f in fams:
        dt, x16, dy16, _ = fam_dt(f, cin, cout)
        q = rb if f == "bf16" else f64
        rnd = lambda t, b: t.to(torch.bfloat16).float() if b else t
        x, dy = rnd(x0, x16), rnd(dy0, dy16)
        for pro in (False, True):
            xin = leaky(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), SLOPE) if pro else x
            xr = q(xin) if f == "bf16" else (leaky(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), SLOPE) if pro else x.double())
            if up:
                xr = F.interpolate(xr, scale_factor=2, mode="nearest")
            wref = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
            bref = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
            F.conv2d(xr, wref, bref, stride=stride, padding=pad).backward(q(dy))
            kw = dict(n=n, hin=hx, win=wx, cin=cin, hout=ho, wout=wo, cout=cout, ks=ks, stride=stride, pad=pad, in_mode=_ffi.IN_UP2 if up else 0,
                      pro_affine=int(pro), pro_slope=SLOPE if pro else 0.0, dt=dt)
            strides = (cin * ks * ks, ks * ks, ks, 1)
            for acc in ((0, 1) if not pro or (ks == 3 and stride == 1 and not up) else (0,)):
                dw, db = run_wgrad(kw, dev(x, x16), dev(dy, dy16), strides, (cout, cin, ks, ks), acc, base, (dev(sc), dev(sh)) if pro else None,
                                   again=f == fam)
                what = f"{f} {form} prologue={pro} accumulate={acc}"
                add_w, add_b = (base[0].double(), base[1].double()) if acc else (0.0, 0.0)
                judge_w(f, oihw(dw, cout, cin, ks), wref.grad + add_w, what + " dW", 1e-3 if pro else 3e-4, res.get(("w", pro, acc)))
                judge_w(f, db, bref.grad + add_b, what + " db", 3e-4, res.get(("b", pro, acc)))
                if f == "fp32":
                    res["w", pro, acc], res["b", pro, acc] = oihw(dw, cout, cin, ks), db


SMALL_CIN = [(c4, *s) for s in NARROW[:2] + [(3, 4, 32, 20, 12)] for c4 in (0, 1)] + [(0, *s) for s in OFFGRID[:4] + OFFGRID[-2:]]


@pytest.mark.parametrize("c4,n,cin,cout,h,w", SMALL_CIN, ids=["-".join(map(str, s)) for s in SMALL_CIN])
def test_wgrad_small_cin_plain_and_k_packed(n, cin, cout, h, w, c4):
    """the <= 4-channel first layers: the plain path and the row-packed CTL_IN_C4 form (fp32 family), padded cin fragment; cin 8 and 12
    (a padded cin fragment too) on the plain path, between foreign gradient ranges and with accumulate 0 / 1"""
    g = gen_for(n, cin, cout, h, w, 40 + c4)
    x, dy = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cout, h, w, generator=g)
    wref = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    bref = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wref, bref, padding=1).backward(dy.double())
    kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3, in_mode=_ffi.IN_C4 if c4 else 0)
    base = (torch.randn(cout, cin, 3, 3, generator=g), torch.randn(cout, generator=g))
    xd = dev(x) if cin > 1 else x.to(DEV).contiguous()
    for acc in (0, 1):
        dw, db = run_wgrad(kw, xd, dev(dy), (cin * 9, 9, 3, 1), (cout, cin, 3, 3), acc, base)
        judge_w("fp32", oihw(dw, cout, cin, 3), wref.grad + (base[0].double() if acc else 0.0), f"first-layer dW (c4 {c4}, accumulate {acc})")
        judge_w("fp32", db, bref.grad + (base[1].double() if acc else 0.0), f"first-layer db (c4 {c4}, accumulate {acc})")
    if c4:                                                      # ... with the virtual output gradient (the encoder's first conv pair)
        u = torch.randn(n, cout, h, w, generator=g)
        coef = torch.stack([torch.rand(1, cout, generator=g) + 0.5, torch.randn(1, cout, generator=g) * 0.3, torch.randn(1, cout, generator=g) * 0.3], 1).contiguous()
        virt = coef[0, 0].double().view(1, -1, 1, 1) * dy.double() + coef[0, 1].double().view(1, -1, 1, 1) * u.double() + coef[0, 2].double().view(1, -1, 1, 1)
        wv = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
        bv = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), wv, bv, padding=1).backward(virt)
        dw, db = run_wgrad(kw, xd, dev(dy), (cin * 9, 9, 3, 1), (cout, cin, 3, 3), dy2=dev(u), coef=dev(coef))
        judge_w("fp32", oihw(dw, cout, cin, 3), wv.grad, "first-layer dW with a virtual output gradient")
        judge_w("fp32", db, bv.grad, "first-layer db with a virtual output gradient")


@pytest.mark.parametrize("form,n,cin,cout,h,w,fam", wgrad_cases(RAGGED + PC, ["3x3", "3x3_up2"]))
def test_wgrad_virtual_output_gradient(form, n, cin, cout, h, w, fam):
    """ctl_conv_wgrad_ex with dy2: the output gradient is A*dy + B*dy2 + C per BatchNorm group; the bias gradient is its sum.  The weight
    tensor is scattered in the [Cin][Cout][3][3] layout (strides of a transposed weight), one and two groups."""
    fams = ("fp32", "x3") if fam == "x3" else (fam,)
    g = gen_for(n, cin, cout, h, w, 50)
    up = FORMS[form][2]
    hx, wx = h, w
    if up:
        h, w = 2 * h, 2 * w
    for groups in ([1, 2] if n % 2 == 0 else [1]):
        if groups * cout > 256:
            continue
        gi = group_index(n, groups)
        x0, g0, u0 = torch.randn(n, cin, hx, wx, generator=g), torch.randn(n, cout, h, w, generator=g), torch.randn(n, cout, h, w, generator=g)
        coef = torch.stack([torch.rand(groups, cout, generator=g) + 0.5, torch.randn(groups, cout, generator=g) * 0.3,
                            torch.randn(groups, cout, generator=g) * 0.3], 1).contiguous()
        res = {}
        for f in fams:
            b16 = f == "bf16"
            dt, x16, dy16, _ = fam_dt(f, cin, cout)
            rnd = lambda t, b: t.to(torch.bfloat16).float() if b else t
            x, gt, u = rnd(x0, x16), rnd(g0, dy16), rnd(u0, dy16)
            A, B, C = (per_group(coef[:, k], gi) for k in range(3))
            virt = rb(A * gt + B * u + C) if b16 else (A.double() * gt.double() + B.double() * u.double() + C.double())
            wref = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
            bref = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
            xr = rb(x) if b16 else x.double()
            F.conv2d(F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr, wref, bref, padding=1).backward(virt)
            kw = dict(n=n, hin=hx, win=wx, cin=cin, hout=h, wout=w, cout=cout, ks=3, groups=groups, in_mode=_ffi.IN_UP2 if up else 0, dt=dt)
            dw, db = run_wgrad(kw, dev(x, x16), dev(gt, dy16), (9, cout * 9, 3, 1), (cin, cout, 3, 3), dy2=dev(u, dy16), coef=dev(coef), again=f == fam)
            what = f"{f} virtual output gradient groups={groups}"
            judge_w(f, dw.view(cin, cout, 3, 3).transpose(0, 1), wref.grad, what + " dW", 1.5e-3, res.get("w"))
            judge_w(f, db, bref.grad, what + " db", 1e-3, res.get("b"))
            if f == "fp32":
                res["w"], res["b"] = dw.view(cin, cout, 3, 3).transpose(0, 1), db


@pytest.mark.parametrize("fam", ["fp32", "bf16"])
@pytest.mark.parametrize("n,cin,cout,h,w", [s for s in OFFGRID if s[2] % 16])
def test_wgrad_virtual_output_gradient_is_refused_off_grid(n, cin, cout, h, w, fam):
    """the two-tensor output gradient stages its coefficients per whole 16-channel cout tile: refused by name at cout 8 / 12 / 20 / 24 / 36 / 40"""
    refused(dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3, dt=fam_dt(fam, cin, cout)[0]), [f"cout {cout}"], two=True, wgrad=True)


def test_wgrad_without_a_bias_partial_leaves_db_alone():
    n, cin, cout, h, w = 2, 16, 16, 9, 7
    g = gen_for(n, cin, cout, h, w, 60)
    x, dy = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cout, h, w, generator=g)
    wref = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wref, padding=1).backward(dy.double())
    kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3)
    dw, _ = run_wgrad(kw, dev(x), dev(dy), (cin * 9, 9, 3, 1), (cout, cin, 3, 3), want_bias=False)
    judge_w("fp32", oihw(dw, cout, cin, 3), wref.grad, "dW without a bias gradient")


# ------------------------------------------------------------------------------------------------ grouped launches
MEMBERS = [(8, 32, 32, 16, 16), (8, 64, 32, 20, 28), (8, 128, 128, 8, 8)]


def _member(m, fam, g, up=0, two=0, ks=3, stride=1):
    """up: behind a nearest up-sampling; two: the virtual output gradient A*dy + B*u + C"""
    n, cin, cout, h, w = m
    b16 = fam == "bf16"
    rnd = (lambda t: t.to(torch.bfloat16).float()) if b16 else (lambda t: t)
    pad = 1 if ks == 3 else 0
    if ks == 2:
        h, w = 2 * h, 2 * w                                     # 2x2 stride 2: the input is the fine tensor
    hi, wi = (2 * h, 2 * w) if up else (h, w)
    ho, wo = (hi + 2 * pad - ks) // stride + 1, (wi + 2 * pad - ks) // stride + 1
    x, dy = rnd(torch.randn(n, cin, h, w, generator=g)), rnd(torch.randn(n, cout, ho, wo, generator=g))
    u = coef = None
    dyv = dy.double()
    if two:
        u = rnd(torch.randn(n, cout, ho, wo, generator=g))
        coef = torch.stack([torch.rand(1, cout, generator=g) + 0.5, torch.randn(1, cout, generator=g) * 0.3, torch.randn(1, cout, generator=g) * 0.3], 1).contiguous()
        v32 = coef[0, 0].view(1, -1, 1, 1) * dy + coef[0, 1].view(1, -1, 1, 1) * u + coef[0, 2].view(1, -1, 1, 1)
        dyv = rb(v32) if b16 else (coef[0, 0].double().view(1, -1, 1, 1) * dy.double() + coef[0, 1].double().view(1, -1, 1, 1) * u.double()
                                   + coef[0, 2].double().view(1, -1, 1, 1))
    wref = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    bref = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    xr = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up else x.double()
    F.conv2d(xr, wref, bref, stride=stride, padding=pad).backward(dyv)
    dt = (_ffi.DT_BF16 | _ffi.DT_X16 | _ffi.DT_Y16) if b16 else _ffi.DT_X3
    kw = dict(n=n, hin=h, win=w, cin=cin, hout=ho, wout=wo, cout=cout, ks=ks, stride=stride, pad=pad, in_mode=_ffi.IN_UP2 if up else 0, dt=dt)
    return dict(kw=kw, x=dev(x, b16), dy=dev(dy, b16), u=None if u is None else dev(u, b16), coef=None if coef is None else dev(coef), dw=wref.grad, db=bref.grad,
                x32=dev(x), dy32=dev(dy), u32=None if u is None else dev(u))


@pytest.mark.parametrize("fam", ["x3", "bf16"])
@pytest.mark.parametrize("up,two", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("pick", [(0, 1), (0, 2), (1, 2), (0, 1, 2)])
def test_grouped_wgrad_partials_sized_by_the_planned_splits(pick, up, two, fam):
    """ctl_wgrad_group_plan + ctl_conv_wgrad_group + ctl_wgrad_reduce_batched: every member's partials are Guarded payloads of exactly
    splits[i] * 9 * cin * cout (+ splits[i] * cout) floats; the gradients land in one flat buffer between foreign ranges"""
    g = gen_for(*pick, 70 + 2 * up + two)
    _grouped([_member(MEMBERS[i], fam, g, up, two) for i in pick], fam, two, f"{fam} group {pick}")


# bf16 family: any weight gradient can ride in a stacked launch with others of its kernel instantiation (tile height 8 / 4 rows from
# hout >= 8, one or two cout tiles per block): two members of equal channel counts per instantiation
BF16_PAIRS = {"8rows_2tiles": [(8, 64, 32, 16, 16), (4, 64, 32, 20, 28)], "8rows_1tile": [(8, 32, 16, 16, 16), (4, 32, 16, 20, 28)],
              "4rows_2tiles": [(8, 32, 32, 4, 4), (4, 32, 32, 6, 6)]}


@pytest.mark.parametrize("pair", list(BF16_PAIRS))
@pytest.mark.parametrize("form", ["3x3", "3x3_s2", "1x1", "2x2_s2"])
def test_grouped_bf16_wgrad_of_every_kernel_size(form, pair):
    ks, stride, _ = FORMS[form]
    g = gen_for(ks, stride, len(pair), 80)
    _grouped([_member(m, "bf16", g, 0, 0, ks, stride) for m in BF16_PAIRS[pair]], "bf16", 0, f"bf16 {form} group {pair}")


def _grouped(members, fam, two, label):
    nm = len(members)
    ks = members[0]["kw"]["ks"]
    taps = ks * ks
    descs = np.concatenate([np.atleast_1d(_ffi.conv_desc(**m["kw"])) for m in members])
    classes = [int(lib.ctl_wgrad_group_class(descs[i:i + 1].ctypes.data, two)) for i in range(nm)]
    assert min(classes) >= 0 and len(set(classes)) == 1, f"group classes {classes}: the members cannot share a launch"
    splits = np.zeros(nm, dtype=np.int32)
    check(lib.ctl_wgrad_group_plan(descs.ctypes.data, nm, splits.ctypes.data), "ctl_wgrad_group_plan")
    assert int(splits.min()) >= 1
    gc = GuardedCall(DEV)
    wparts, bparts, sizes = [], [], [NEIGHBOURS[0]]
    for k, (m, sp) in enumerate(zip(members, splits)):
        cin, cout = m["kw"]["cin"], m["kw"]["cout"]
        wparts.append(gc.out(f"w_partial[{k}]", int(sp) * taps * cin * cout, written=False))
        bparts.append(gc.out(f"b_partial[{k}]", int(sp) * cout, written=False))
        sizes += [cout * cin * taps, cout, NEIGHBOURS[1]]
    gen = torch.Generator().manual_seed(nm)
    foreign = {i: torch.randn(s, generator=gen).to(DEV) for i, s in enumerate(sizes) if i % 3 == 0}

    def init(f):
        for i, t in foreign.items():
            f.range(i).copy_(t)

    grad = gc.flat("grad", sizes, written=[i for i in range(len(sizes)) if i % 3], init=init)
    base = min(b.ptr for b in wparts + bparts)
    recs = []
    for k, (m, sp) in enumerate(zip(members, splits)):
        cin, cout = m["kw"]["cin"], m["kw"]["cout"]
        recs.append([(wparts[k].ptr - base) // 4, (bparts[k].ptr - base) // 4, grad.offsets[1 + 3 * k], grad.offsets[2 + 3 * k], int(sp), taps | (ks << 8), cin, cout,
                     cin, cout, cin * taps, taps, ks, 1, 0, 0])
    table = torch.tensor(recs, dtype=torch.int64, device=DEV)
    max_blocks = max(-(-(taps * r[6] * r[7] + r[7]) // (64 if r[4] <= 64 else 8)) for r in recs)
    arr = lambda ps: (ctypes.c_void_p * nm)(*ps)
    none = (ctypes.c_void_p * nm)()

    def launch():
        check(lib.ctl_conv_wgrad_group(nm, descs.ctypes.data, splits.ctypes.data, arr([m["x"].data_ptr() for m in members]), none, none,
                                       arr([m["dy"].data_ptr() for m in members]), arr([m["u"].data_ptr() for m in members]) if two else none,
                                       arr([m["coef"].data_ptr() for m in members]) if two else none, arr([b.ptr for b in wparts]), arr([b.ptr for b in bparts]),
                                       ops.stream_ptr()), "ctl_conv_wgrad_group")
        check(lib.ctl_wgrad_reduce_batched(base, grad.ptr, table.data_ptr(), nm, max_blocks, ops.stream_ptr()), "ctl_wgrad_reduce_batched")

    def foreign_intact():
        for i, t in foreign.items():
            assert torch.equal(grad.range(i).view(torch.int32), t.view(torch.int32)), f"the foreign gradient range {i} was changed"

    gc.run(launch)
    foreign_intact()
    for b in wparts + bparts:                                   # cin and cout are multiples of 16 here: no padding, every planned split is consumed
        b.check_written()
    for k, m in enumerate(members):
        cin, cout = m["kw"]["cin"], m["kw"]["cout"]
        dw, db = grad.range(1 + 3 * k).cpu().view(cout, cin, ks, ks), grad.range(2 + 3 * k).cpu()
        what = f"{label} member {k} ({int(splits[k])} splits)"
        if fam == "x3":                                         # next to the fp32-MFMA kernel on the same member
            dw0, db0 = torch.zeros(cout, cin, 3, 3, device=DEV), torch.zeros(cout, device=DEV)
            ops.conv_wgrad(_ffi.conv_desc(**dict(m["kw"], dt=0)), m["x32"], m["dy32"], dw0, (cin * 9, 9, 3, 1), dbias=db0, dy2=m["u32"], dy_coef=m["coef"])
            judge_w("x3", dw, m["dw"], what + " dW", got32=dw0)
            judge_w("x3", db, m["db"], what + " db", got32=db0)
        else:
            judge_w("bf16", dw, m["dw"], what + " dW", 1.5e-3 if two else 3e-4)      # (the rules of test_wgrad_virtual_output_gradient, tests/test_bf16_gpu.py)
            judge_w("bf16", db, m["db"], what + " db", 1e-3 if two else 3e-4)
    gc.rerun(launch)
    foreign_intact()


# ------------------------------------------------------------------------------------------------ the checks bite on the device too
def test_a_w_partial_one_row_short_is_reported_as_exactly_the_missing_bytes():
    """w_partial declared one row (cout floats) shorter than ctl_wgrad_partial_floats says: the last split's last row lands in the back
    guard of the test's own allocation (256 KiB; nothing faults) and check_guards reports exactly those bytes"""
    n, cin, cout, h, w = 2, 16, 16, 9, 7
    g = gen_for(n, cin, cout, h, w, 98)
    x, dy = dev(torch.randn(n, cin, h, w, generator=g) + 2.0), dev(torch.randn(n, cout, h, w, generator=g) + 2.0)      # (sums far from zero)
    d = _ffi.conv_desc(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3)
    dp = _ffi.desc_ptr(d)
    nw, nb = int(lib.ctl_wgrad_partial_floats(dp)), int(lib.ctl_wgrad_bias_partial_floats(dp))
    wpart, bpart = Guarded(nw - cout, torch.float32, DEV, name="w_partial"), Guarded(nb, torch.float32, DEV, name="b_partial")
    check(lib.ctl_conv_wgrad_ex(dp, x.data_ptr(), None, None, dy.data_ptr(), None, None, wpart.ptr, bpart.ptr, ops.stream_ptr()))
    bpart.check_guards()
    bpart.check_written()
    wpart.check_written()
    v = wpart.guard_violations()
    row = wpart._back()[:4 * cout].cpu()
    assert bool((row.view(torch.int32) != 0x5A5A5A5A).all()), "a float of the missing row was not written"
    same = int((row == 0x5A).sum())                             # a written byte that equals the guard pattern cannot count as touched
    assert len(v) == 1 and v[0]["side"] == "back" and wpart.nbytes <= v[0]["first"] and v[0]["last"] < wpart.nbytes + 4 * cout, v
    assert v[0]["count"] == 4 * cout - same, (v, same)
    with pytest.raises(AssertionError):
        wpart.check_guards()
