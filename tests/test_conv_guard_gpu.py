"""ctl_conv_forward_ex behind guard bands (oracle/guarded.py): production packs activations and statistics partials back to back at
256-byte granularity, so a ragged last tile that writes past its tensor, or a statistics row nobody wrote, lands in (or is read from) a
neighbour there -- and in nothing at all in a test that gives every output an allocator block of its own.

Every case: each written buffer (y, stats_partial, xout, pool) is a Guarded sized exactly by the tensor shape or the library's size query
and poisoned with NaN bits; after the call both guards must be intact and every element written; the result is held to an fp64 CPU
reference by the rule of the family's own file (tests/test_kernels_gpu.py: 2e-4; tests/test_x3_gpu.py: errs() next to the fp32 kernel;
tests/test_bf16_gpu.py: same rounding points, 3e-4 / 1e-3 / 2^-8); then the buffers are poisoned again, the identical call is repeated and
the payloads must be bit-identical.  The shapes are the smallest that leave every tile dimension ragged (tiles are 4 or 8 high, 16 or 32
wide; the X3 producer / consumer form works on 32x32 blocks) and include the padded-channel tiles."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check  # noqa: E402
from oracle.guarded import Guarded  # noqa: E402

from oracle.guard_conv import (BF, DEV, FAMILIES, FIRST, NARROW, OFFGRID, OFFGRID_EVEN, OFFGRID_TILED, PC, RAGGED, SLOPE, TILED, TILED_UP, chan_ok, close16, dev,  # noqa: E402
                               f64, fam_dt, gen_for, group_index, judge, judge_sums, each_family, fam_cases, leaky, need, pack, pack_dgrad, pack_fwd, pack_phases,
                               per_group, rb, ref_sums, refused, run_conv, x3_ok)


# ------------------------------------------------------------------------------------------------ 3x3 stride 1
@pytest.mark.parametrize("n,cin,cout,h,w,fam", fam_cases(RAGGED + PC + NARROW + TILED + FIRST + [(8, 128, 128, 32, 32)] + OFFGRID + OFFGRID_TILED, 3))
def test_conv3x3_s1_bias_stats_prologue_groups(n, cin, cout, h, w, fam):
    """bias + CTL_EPI_STATS; the pro_affine = 1 prologue; both again with two BatchNorm groups on the even-n cases.  bf16 family: the
    storage combinations of tests/test_bf16_gpu.py (x / y as bf16 or fp32)."""
    fams = need(fam, cin, cout, 3)
    g = gen_for(n, cin, cout, h, w)
    x0 = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    c4 = fam == "fp32" and cin <= 4                         # the K-packed first-layer form (CTL_IN_C4) next to the plain path
    combos = [(True, True), (False, False), (False, True), (True, False)] if fam == "bf16" and (n, cin, cout, h, w) in RAGGED else [(True, True)]
    base0 = torch.randn(n, cout, h, w, generator=g)
    for groups in ([1, 2] if n % 2 == 0 else [1]):
        gi = group_index(n, groups)
        sc, sh = torch.rand(groups, cin, generator=g) + 0.5, torch.randn(groups, cin, generator=g) * 0.3
        for x16w, y16w in combos:
            for in_mode in ([0, _ffi.IN_C4] if c4 else [0]):
                res = {}
                for f in each_family(fams, fam):
                    dt, x16, y16, _ = fam_dt(f, cin, cout, x16w, y16w)
                    q = rb if f == "bf16" else f64
                    x = x0.to(torch.bfloat16).float() if x16 else x0
                    xd = dev(x, x16) if cin > 1 else (x.to(DEV).to(torch.bfloat16 if x16 else torch.float32).contiguous())
                    wp = pack(f, wt, [(0, cout, cin, 3, 0, (cin * 9, 9, 3, 1), 4)]) if in_mode else pack_fwd(f, wt)
                    kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3, in_mode=in_mode, groups=groups, dt=dt,
                              epi_flags=_ffi.EPI_BIAS | _ffi.EPI_STATS)
                    o = run_conv(kw, xd, wp, (n, cout, h, w), y16, want_stats=True, bias=dev(b))
                    ref = F.conv2d(q(x), q(wt), b.double(), padding=1)
                    what = f"{f} conv3x3 groups={groups} in_mode={in_mode} x16={x16} y16={y16}"
                    judge(f, o["y"], ref, what, b16out=y16, got32=res.get("y"))
                    want = ref_sums(ref, ref, gi, groups)
                    judge_sums(f, o["stats"].sum(1), want, what + " statistics", "stats")
                    if f == "fp32":
                        res["y"] = o["y"]
                    if in_mode:
                        continue                                # (the prologue is not part of the K-packed form)
                    kw2 = dict(kw, epi_flags=_ffi.EPI_BIAS, pro_affine=1, pro_slope=SLOPE)
                    o2 = run_conv(kw2, xd, wp, (n, cout, h, w), y16, bias=dev(b), pro_scale=dev(sc), pro_shift=dev(sh))
                    pro = leaky(x * per_group(sc, gi) + per_group(sh, gi), SLOPE)      # fp32 prologue, THEN the operand rounding
                    ref2 = F.conv2d(q(pro), q(wt), b.double(), padding=1) if f == "bf16" else \
                        F.conv2d(leaky(x.double() * per_group(sc, gi).double() + per_group(sh, gi).double(), SLOPE), wt.double(), b.double(), padding=1)
                    judge(f, o2["y"], ref2, what + " + prologue", pro=True, b16out=y16, got32=res.get("y2"))
                    if f == "fp32":
                        res["y2"] = o2["y"]
                    if groups == 1 and x16w == y16w:            # accumulate into an existing output (the 3x3 data gradients)
                        base = base0.to(torch.bfloat16).float() if y16 else base0
                        o3 = run_conv(dict(kw, epi_flags=_ffi.EPI_ACCUM), xd, wp, (n, cout, h, w), y16, y_init=base)
                        judge(f, o3["y"], F.conv2d(q(x), q(wt), padding=1) + base.double(), what + " + accumulate", b16out=y16, got32=res.get("y3"))
                        if f == "fp32":
                            res["y3"] = o3["y"]


# ------------------------------------------------------------------------------------------------ stride 2, zero insertion, up-sampling
@pytest.mark.parametrize("n,cin,cout,h,w,fam", fam_cases(RAGGED + PC + NARROW + [(2, 16, 32, 32, 32), (16, 16, 32, 96, 128)] + OFFGRID + [(16, 8, 8, 96, 128)], 3))
def test_conv3x3_s2_and_zero_insert_data_gradient(n, cin, cout, h, w, fam):
    """3x3 stride 2 on odd sizes, and its data gradient as a 3x3 conv over the zero-inserted dy (CTL_IN_ZINS2; X3: even sizes, as in
    tests/test_x3_gpu.py)."""
    fams = need(fam, cin, cout, 3)
    g = gen_for(n, cin, cout, h, w, 2)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    x0 = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    dy0 = torch.randn(n, cout, ho, wo, generator=g)
    res = {}
    for f in each_family(fams, fam):
        dt, x16, y16, _ = fam_dt(f, cin, cout)
        q = rb if f == "bf16" else f64
        x = x0.to(torch.bfloat16).float() if x16 else x0
        xd = dev(x, x16) if cin > 1 else x.to(DEV).contiguous()
        kw = dict(n=n, hin=h, win=w, cin=cin, hout=ho, wout=wo, cout=cout, ks=3, stride=2, epi_flags=_ffi.EPI_BIAS, dt=dt)
        o = run_conv(kw, xd, pack_fwd(f, wt), (n, cout, ho, wo), y16, bias=dev(b))
        judge(f, o["y"], F.conv2d(q(x), q(wt), b.double(), stride=2, padding=1), f"{f} conv3x3 s2", b16out=y16, got32=res.get("y"))
        if f == "fp32":
            res["y"] = o["y"]
        # data gradient: conv over the zero-inserted dy with flipped / transposed weights: [n, cout, ho, wo] -> [n, cin, h, w]
        if cin == 1 or (fam == "x3" and (h % 2 or w % 2 or not x3_ok(cout, cin, 3))):
            continue
        if not chan_ok(cout, cin):                              # cout 20 / 24 / 36 / 40 is no input channel count: the data gradient is refused
            refused(dict(n=n, hin=ho, win=wo, cin=cout, hout=h, wout=w, cout=cin, ks=3, in_mode=_ffi.IN_ZINS2, dt=fam_dt(f, 16, cin)[0]), [f"got {cout}"])
            continue
        dtz, dy16, dx16, _ = fam_dt(f, cout, cin)
        dy = dy0.to(torch.bfloat16).float() if dy16 else dy0
        kwz = dict(n=n, hin=ho, win=wo, cin=cout, hout=h, wout=w, cout=cin, ks=3, in_mode=_ffi.IN_ZINS2, dt=dtz)
        oz = run_conv(kwz, dev(dy, dy16), pack_dgrad(f, wt), (n, cin, h, w), dx16)
        refz = F.conv_transpose2d(q(dy), q(wt), stride=2, padding=1, output_padding=(h - (2 * ho - 1), w - (2 * wo - 1)))
        judge(f, oz["y"], refz, f"{f} zero-insert data gradient", b16out=dx16, got32=res.get("dx"))
        if f == "fp32":
            res["dx"] = oz["y"]


@pytest.mark.parametrize("n,cin,cout,h,w,fam", fam_cases(RAGGED + PC + NARROW[2:] + TILED_UP + OFFGRID, 3))
def test_conv3x3_on_nearest_upsampled_input(n, cin, cout, h, w, fam):
    """CTL_IN_UP2 3x3 with the residual + LeakyReLU epilogue (X3, bf16) or plain (all)"""
    fams = need(fam, cin, cout, 3)
    g = gen_for(n, cin, cout, h, w, 3)
    x0 = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    v0 = torch.randn(n, cout, 2 * h, 2 * w, generator=g)
    rs, rh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    res = {}
    for f in each_family(fams, fam):
        dt, x16, y16, r16 = fam_dt(f, cin, cout)
        q = rb if f == "bf16" else f64
        x, v = (x0.to(torch.bfloat16).float() if x16 else x0), (v0.to(torch.bfloat16).float() if r16 else v0)
        kw = dict(n=n, hin=h, win=w, cin=cin, hout=2 * h, wout=2 * w, cout=cout, ks=3, in_mode=_ffi.IN_UP2, epi_flags=_ffi.EPI_RES, epi_act=_ffi.ACT_LEAKY,
                  epi_slope=SLOPE, dt=dt)
        o = run_conv(kw, dev(x, x16), pack_fwd(f, wt), (n, cout, 2 * h, 2 * w), y16, res=dev(v, r16), res_scale=dev(rs), res_shift=dev(rh))
        up = F.interpolate(q(x), scale_factor=2, mode="nearest")
        ref = leaky(F.conv2d(up, q(wt), padding=1) + v.double() * rs.double().view(1, -1, 1, 1) + rh.double().view(1, -1, 1, 1), SLOPE)
        judge(f, o["y"], ref, f"{f} conv3x3(up2) + residual + leaky", b16out=y16, got32=res.get("y"))
        o0 = run_conv(dict(kw, epi_flags=0, epi_act=0), dev(x, x16), pack_fwd(f, wt), (n, cout, 2 * h, 2 * w), y16)
        judge(f, o0["y"], F.conv2d(up, q(wt), padding=1), f"{f} conv3x3(up2)", b16out=y16, got32=res.get("y0"))
        if f == "fp32":
            res["y"], res["y0"] = o["y"], o0["y"]


# ------------------------------------------------------------------------------------------------ 1x1 and the scattered forms
@pytest.mark.parametrize("fam", ["fp32", "bf16"])
@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("n,cin,cout,h,w", RAGGED + PC + NARROW[2:] + [(16, 16, 16, 32, 64), (8, 16, 32, 48, 64)] + OFFGRID + OFFGRID_TILED[:1])
def test_conv1x1_residual_leaky_and_accumulate(n, cin, cout, h, w, up, fam):
    g = gen_for(n, cin, cout, h, w, 4 + up)
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    dt, x16, y16, r16 = fam_dt(fam, cin, cout)
    q = rb if fam == "bf16" else f64
    x = torch.randn(n, cin, h, w, generator=g)
    v = torch.randn(n, cout, ho, wo, generator=g)
    x, v = (x.to(torch.bfloat16).float() if x16 else x), (v.to(torch.bfloat16).float() if r16 else v)
    wt = torch.randn(cout, cin, 1, 1, generator=g) * 0.3
    b = torch.randn(cout, generator=g)
    rs, rh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    wp = pack_fwd(fam, wt)
    kw = dict(n=n, hin=h, win=w, cin=cin, hout=ho, wout=wo, cout=cout, ks=1, in_mode=_ffi.IN_UP2 if up else 0, dt=dt,
              epi_flags=_ffi.EPI_BIAS | _ffi.EPI_RES, epi_act=_ffi.ACT_LEAKY, epi_slope=SLOPE)
    o = run_conv(kw, dev(x, x16), wp, (n, cout, ho, wo), y16, bias=dev(b), res=dev(v, r16), res_scale=dev(rs), res_shift=dev(rh))
    xi = F.interpolate(q(x), scale_factor=2, mode="nearest") if up else q(x)
    conv = F.conv2d(xi, q(wt))
    ref = leaky(conv + b.double().view(1, -1, 1, 1) + v.double() * rs.double().view(1, -1, 1, 1) + rh.double().view(1, -1, 1, 1), SLOPE)
    judge(fam, o["y"], ref, f"{fam} conv1x1 + residual + leaky (up {up})", b16out=y16)
    base = torch.randn(n, cout, ho, wo, generator=g)
    base = base.to(torch.bfloat16).float() if y16 else base
    kw3 = dict(kw, epi_flags=_ffi.EPI_ACCUM, epi_act=0)
    o3 = run_conv(kw3, dev(x, x16), wp, (n, cout, ho, wo), y16, y_init=base)
    judge(fam, o3["y"], conv + base.double(), f"{fam} conv1x1 accumulate (up {up})", b16out=y16)
    kw2 = dict(kw, epi_flags=_ffi.EPI_BIAS, epi_act=_ffi.ACT_SIGMOID)
    o2 = run_conv(kw2, dev(x, x16), wp, (n, cout, ho, wo), y16, bias=dev(b))
    judge(fam, o2["y"], torch.sigmoid(conv + b.double().view(1, -1, 1, 1)), f"{fam} conv1x1 + sigmoid (up {up})", b16out=y16)


@pytest.mark.parametrize("fam", ["fp32", "bf16"])
@pytest.mark.parametrize("n,cin,cout,h,w", RAGGED + PC + [(8, 16, 16, 64, 64)] + [s for s in OFFGRID if 8 in s[1:3]])
def test_conv_transpose2x2_scatter(n, cin, cout, h, w, fam):
    """ConvTranspose2d k2 s2 as four scattered 1x1 problems (nsub = 4): every output pixel belongs to exactly one of them"""
    g = gen_for(n, cin, cout, h, w, 6)
    dt, x16, y16, _ = fam_dt(fam, cin, cout)
    q = rb if fam == "bf16" else f64
    x = torch.randn(n, cin, h, w, generator=g)
    x = x.to(torch.bfloat16).float() if x16 else x
    wt = torch.randn(cin, cout, 2, 2, generator=g) * 0.2   # [Cin][Cout][2][2]
    b = torch.randn(cout, generator=g)
    wp = pack(fam, wt, [(z, cout, cin, 1, 0, (4, cout * 4, 0, 0), 0) for z in range(4)])
    kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=1, epi_flags=_ffi.EPI_BIAS, out_h=2 * h, out_w=2 * w, out_sy=2, out_sx=2, nsub=4,
              out_sub=1, dt=dt)
    o = run_conv(kw, dev(x, x16), wp, (n, cout, 2 * h, 2 * w), y16, bias=dev(b))
    judge(fam, o["y"], F.conv_transpose2d(q(x), q(wt), b.double(), stride=2), f"{fam} ConvTranspose2d forward", b16out=y16)


def _phase_reference(x, wt, b, q, n, cin, cout, h, w):
    """conv3x3(up2(x)) as four 2x2 convs whose weights are combined in fp32 and then rounded as the family rounds them"""
    ref = torch.zeros(n, cout, 2 * h, 2 * w, dtype=torch.float64)
    xp = F.pad(q(x), (1, 1, 1, 1))
    for a in range(2):
        for bb in range(2):
            k = torch.zeros(cout, cin, 2, 2)
            for kh in range(3):
                for kw_ in range(3):
                    k[:, :, (a + kh + 1) // 2 - a, (bb + kw_ + 1) // 2 - bb] += wt[:, :, kh, kw_]
            ref[:, :, a::2, bb::2] = F.conv2d(xp[:, :, a:a + h + 1, bb:bb + w + 1], q(k)) + b.double().view(1, -1, 1, 1)
    return ref


@pytest.mark.parametrize("n,cin,cout,h,w,fam", fam_cases(RAGGED + PC + [(8, 16, 16, 64, 64)] + OFFGRID, 2))
def test_phase_convs_pad2_and_pad0(n, cin, cout, h, w, fam):
    """the four 2x2 phase problems (nsub = 4): pad code 2 = conv3x3 on a nearest-upsampled input, with bias and statistics; pad code 0 =
    the data gradient of a stride-2 3x3 conv"""
    fams = need(fam, cin, cout, 2)
    g = gen_for(n, cin, cout, h, w, 7)
    x0 = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    ws = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    dy0 = torch.randn(n, cout, h, w, generator=g)
    res = {}
    for f in each_family(fams, fam):
        dt, x16, y16, _ = fam_dt(f, cin, cout)
        q = rb if f == "bf16" else f64
        x = x0.to(torch.bfloat16).float() if x16 else x0
        kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=2, stride=1, pad=2, nsub=4, out_h=2 * h, out_w=2 * w, out_sy=2, out_sx=2,
                  out_sub=1, epi_flags=_ffi.EPI_BIAS | _ffi.EPI_STATS, dt=dt)
        o = run_conv(kw, dev(x, x16), pack_phases(f, wt, cout, cin, (cin * 9, 9, 3, 1), 2), (n, cout, 2 * h, 2 * w), y16, want_stats=True, bias=dev(b))
        ref = _phase_reference(x, wt, b, q, n, cin, cout, h, w)
        judge(f, o["y"], ref, f"{f} phase forward of conv3x3(up2(x))", b16out=y16, got32=res.get("y"))
        want = torch.stack([ref.sum((0, 2, 3)), (ref ** 2).sum((0, 2, 3))])
        got = o["stats"].sum(1)[0]
        assert bool(torch.isfinite(got).all()), "phase statistics: non-finite partial sums"
        assert float((got[1] - want[1]).abs().max()) <= 2e-4 * float(want[1].max()), f"{f} phase statistics (sum of squares)"
        if f == "fp32":
            res["y"] = o["y"]
            assert float((got[0] - want[0]).abs().max()) <= 2e-4 * float(want[0].abs().max()) + 1e-2, "phase statistics (sum)"
        # data gradient of conv3x3 s2 on a [2h, 2w] input: dy [n, cout, h, w] -> dx [n, cin, 2h, 2w]; plain, and with the CTL_EPI_BNBWD
        # epilogue (dx is dL/da of a = leaky(BN(u)): the partials hold (sum g, sum g*u))
        if f == "x3" and not x3_ok(cout, cin, 2):
            continue
        if not chan_ok(cout, cin):                              # (cout 20 / 24 / 36 / 40 is no input channel count)
            refused(dict(n=n, hin=h, win=w, cin=cout, hout=h, wout=w, cout=cin, ks=2, stride=1, pad=0, nsub=4, out_h=2 * h, out_w=2 * w, out_sy=2, out_sx=2,
                         out_sub=1, dt=fam_dt(f, 16, cin)[0]), [f"got {cout}"])
            continue
        dt2, dy16, dx16, r16 = fam_dt(f, cout, cin)
        rnd = (lambda t: t.to(torch.bfloat16).float()) if f == "bf16" else (lambda t: t)
        dy = rnd(dy0) if dy16 else dy0
        kw2 = dict(n=n, hin=h, win=w, cin=cout, hout=h, wout=w, cout=cin, ks=2, stride=1, pad=0, nsub=4, out_h=2 * h, out_w=2 * w, out_sy=2, out_sx=2,
                   out_sub=1, dt=dt2)
        wp2 = pack_phases(f, ws, cin, cout, (9, cin * 9, 3, 1), 3)
        o2 = run_conv(kw2, dev(dy, dy16), wp2, (n, cin, 2 * h, 2 * w), dx16)
        ref2 = F.conv_transpose2d(q(dy), q(ws), stride=2, padding=1, output_padding=1)
        judge(f, o2["y"], ref2, f"{f} phase data gradient of conv3x3 s2", b16out=dx16, got32=res.get("dx"))
        o3 = None
        if cin % 16 == 0 and f == "bf16" and cout % 16 != 0:      # (bf16 family: CTL_EPI_BNBWD takes bf16-stored tensors, whole 16-channel tiles on both sides)
            refused(dict(kw2, epi_flags=_ffi.EPI_BNBWD | _ffi.EPI_STATS, epi_slope=SLOPE), [f"cin {cout}"])
        elif cin % 16 == 0:
            gu = torch.Generator().manual_seed(cin + h)
            u = torch.randn(n, cin, 2 * h, 2 * w, generator=gu)
            u = rnd(u) if r16 else u
            rs, rh = torch.rand(1, cin, generator=gu) + 0.5, torch.randn(1, cin, generator=gu) * 0.3
            kw3 = dict(kw2, epi_flags=_ffi.EPI_BNBWD | _ffi.EPI_STATS, epi_slope=SLOPE)
            o3 = run_conv(kw3, dev(dy, dy16), wp2, (n, cin, 2 * h, 2 * w), dx16, want_stats=True, res=dev(u, r16), res_scale=dev(rs), res_shift=dev(rh))
            ref3 = ref2 * torch.where(u * rs.view(1, -1, 1, 1) + rh.view(1, -1, 1, 1) > 0, 1.0, SLOPE).double()
            judge(f, o3["y"], ref3, f"{f} phase data gradient + CTL_EPI_BNBWD", b16out=dx16, got32=res.get("dx3"))
            judge_sums(f, o3["stats"].sum(1), ref_sums(ref3, u.double(), group_index(n, 1), 1), f"{f} phase CTL_EPI_BNBWD partial sums", "bnbwd")
        if f == "fp32":
            res["dx"], res["dx3"] = o2["y"], None if o3 is None else o3["y"]


@pytest.mark.parametrize("n,cin,cout,h,w,fam", fam_cases([(2, 64, 32, 24, 20), (8, 128, 64, 20, 28), (6, 64, 96, 36, 52), (2, 16, 16, 10, 6), (2, 32, 48, 18, 22), (2, 16, 4, 18, 22), (16, 16, 16, 96, 128), (16, 16, 32, 96, 128)] + OFFGRID_EVEN, 4))
def test_conv4x4_s2_and_conv2x2_s2_on_even_sizes(n, cin, cout, h, w, fam):
    fams = need(fam, cin, cout, 4)
    g = gen_for(n, cin, cout, h, w, 8)
    x0 = torch.randn(n, cin, h, w, generator=g)
    k4 = torch.randn(cout, cin, 4, 4, generator=g) * 0.2
    k2 = torch.randn(cout, cin, 2, 2, generator=g) * 0.3
    base0 = torch.randn(n, cout, h // 2, w // 2, generator=g)
    res = {}
    for f in each_family(fams, fam):
        dt, x16, y16, _ = fam_dt(f, cin, cout)
        q = rb if f == "bf16" else f64
        x = x0.to(torch.bfloat16).float() if x16 else x0
        base = base0.to(torch.bfloat16).float() if y16 else base0
        kw4 = dict(n=n, hin=h, win=w, cin=cin, hout=h // 2, wout=w // 2, cout=cout, ks=4, stride=2, epi_flags=_ffi.EPI_ACCUM, dt=dt)
        o = run_conv(kw4, dev(x, x16), pack_fwd(f, k4), (n, cout, h // 2, w // 2), y16, y_init=base)
        judge(f, o["y"], F.conv2d(q(x), q(k4), stride=2, padding=1) + base.double(), f"{f} conv4x4 s2 + accumulate", b16out=y16, got32=res.get("y4"))
        o0 = run_conv(dict(kw4, epi_flags=0), dev(x, x16), pack_fwd(f, k4), (n, cout, h // 2, w // 2), y16)
        judge(f, o0["y"], F.conv2d(q(x), q(k4), stride=2, padding=1), f"{f} conv4x4 s2", b16out=y16, got32=res.get("y40"))
        if f == "fp32":
            res["y40"] = o0["y"]
        kw2 = dict(n=n, hin=h, win=w, cin=cin, hout=h // 2, wout=w // 2, cout=cout, ks=2, stride=2, pad=0, dt=dt)
        o2 = run_conv(kw2, dev(x, x16), pack_fwd(f, k2), (n, cout, h // 2, w // 2), y16)
        judge(f, o2["y"], F.conv2d(q(x), q(k2), stride=2), f"{f} conv2x2 s2", b16out=y16, got32=res.get("y2"))
        if f == "fp32":
            res["y4"], res["y2"] = o["y"], o2["y"]


# ------------------------------------------------------------------------------------------------ the backward epilogues / prologues
@pytest.mark.parametrize("n,cin,cout,h,w,fam", fam_cases(RAGGED + PC + TILED, 3))
def test_bnbwd_epilogue_and_bn_backward_prologue(n, cin, cout, h, w, fam):
    """CTL_EPI_BNBWD + CTL_EPI_STATS (y = conv * leaky'(u*scale+shift), partials = (sum y, sum y*u) per group), and the same behind the
    BatchNorm-backward prologue pro_affine = 2 (input = A*x + B*x2 + C) with the `xout` side output; one and two groups."""
    fams = need(fam, cin, cout, 3)
    g = gen_for(n, cin, cout, h, w, 9)
    for groups in ([1, 2] if n % 2 == 0 else [1]):
        if groups * cin > 256:
            continue                                            # (the prologue coefficients sit in a 256-entry LDS table)
        gi = group_index(n, groups)
        gt0, u0 = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cin, h, w, generator=g)
        coef = torch.randn(groups, 3, cin, generator=g) * 0.5
        wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
        u20 = torch.randn(n, cout, h, w, generator=g)
        rs, rh = torch.rand(groups, cout, generator=g) + 0.5, torch.randn(groups, cout, generator=g) * 0.3
        res = {}
        for f in each_family(fams, fam):
            dt, x16, y16, r16 = fam_dt(f, cin, cout)
            b16 = f == "bf16"
            q = rb if b16 else f64
            rnd = (lambda t: t.to(torch.bfloat16).float()) if b16 else (lambda t: t)
            gt, u, u2 = rnd(gt0), rnd(u0), rnd(u20)
            sa = u2 * per_group(rs, gi) + per_group(rh, gi)
            lk = torch.where(sa > 0, 1.0, SLOPE).double()
            wp = pack_fwd(f, wt)
            args = dict(res=dev(u2, r16), res_scale=dev(rs), res_shift=dev(rh))
            # (i) plain input
            kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3, groups=groups, epi_flags=_ffi.EPI_BNBWD | _ffi.EPI_STATS, epi_slope=SLOPE, dt=dt)
            o = run_conv(kw, dev(gt, x16), wp, (n, cout, h, w), y16, want_stats=True, **args)
            ref = F.conv2d(q(gt), q(wt), padding=1) * lk
            what = f"{f} CTL_EPI_BNBWD groups={groups}"
            judge(f, o["y"], ref, what, b16out=y16, got32=res.get("y"))
            judge_sums(f, o["stats"].sum(1), ref_sums(ref, u2.double(), gi, groups), what + " partial sums", "bnbwd")
            # (ii) the virtual input A*g + B*u + C, written out as xout
            A, B, C = (per_group(coef[:, k], gi) for k in range(3))
            virt32 = A * gt + B * u + C
            virt = rb(virt32) if b16 else (A.double() * gt.double() + B.double() * u.double() + C.double())
            kw2 = dict(kw, pro_affine=2)
            xd = dev(gt, x16)
            o2 = run_conv(kw2, xd, wp, (n, cout, h, w), y16, want_stats=True, xout_like=xd, pro_scale=dev(coef), x2=dev(u, x16), **args)
            ref2 = F.conv2d(virt, q(wt), padding=1) * lk
            what = f"{f} pro_affine=2 + CTL_EPI_BNBWD groups={groups}"
            judge(f, o2["y"], ref2, what, pro=True, b16out=y16, got32=res.get("y2"))
            judge_sums(f, o2["stats"].sum(1), ref_sums(ref2, u2.double(), gi, groups), what + " partial sums", "bnbwd")
            if b16:
                close16(o2["xout"], virt, 1e-3, what + " xout", True)
            else:
                assert float((o2["xout"].double() - virt).abs().max()) <= 1e-5 * float(virt.abs().max()), what + " xout"
            # (iii) the prologue alone (statistics epilogue), 3x3 stride 1 and the 4x4 stride-2 pooled data gradient
            kw3 = dict(kw, pro_affine=2, epi_flags=_ffi.EPI_STATS)
            o3 = run_conv(kw3, xd, wp, (n, cout, h, w), y16, want_stats=True, xout_like=xd, pro_scale=dev(coef), x2=dev(u, x16))
            ref3 = F.conv2d(virt, q(wt), padding=1)
            what = f"{f} pro_affine=2 groups={groups}"
            judge(f, o3["y"], ref3, what, pro=True, b16out=y16, got32=res.get("y3"))
            judge_sums(f, o3["stats"].sum(1), ref_sums(ref3, ref3, gi, groups), what + " statistics", "pro2")
            o4 = None
            if h % 2 == 0 and w % 2 == 0 and x3_ok(cin, cout, 4):
                w4 = torch.randn(cout, cin, 4, 4, generator=torch.Generator().manual_seed(cin + cout)) * 0.2
                kw4 = dict(n=n, hin=h, win=w, cin=cin, hout=h // 2, wout=w // 2, cout=cout, ks=4, stride=2, groups=groups, pro_affine=2, dt=dt)
                o4 = run_conv(kw4, xd, pack_fwd(f, w4), (n, cout, h // 2, w // 2), y16, xout_like=xd, pro_scale=dev(coef), x2=dev(u, x16))
                judge(f, o4["y"], F.conv2d(virt, q(w4), stride=2, padding=1), what + " conv4x4 s2", pro=True, b16out=y16, got32=res.get("y4"))
                if b16:
                    close16(o4["xout"], virt, 1e-3, what + " xout of the 4x4 form", True)
                else:
                    assert float((o4["xout"].double() - virt).abs().max()) <= 1e-5 * float(virt.abs().max()), what + " xout of the 4x4 form"
            if f == "fp32":
                res["y"], res["y2"], res["y3"], res["y4"] = o["y"], o2["y"], o3["y"], None if o4 is None else o4["y"]


# ctl_conv_pool_ok needs a tile configuration that gives every wave a row pair (8x16 or 8x32 pixels): 384 / 512 blocks, see TILED
POOL_SHAPES = {(8, 16, 48, 30, 62): "8x16", (8, 16, 48, 58, 66): "8x32"}
TAIL_SHAPES = [(2, 16, 16, 10, 6), (2, 32, 48, 18, 22), (3, 48, 16, 34, 36), (2, 128, 64, 6, 6), (2, 64, 32, 24, 20), (8, 128, 64, 20, 28)] + list(POOL_SHAPES)
TAIL_KS = {"1x1": 1, "1x1_accum": 1, "2x2_s2": 2, "zins_3x3": 3, "phase_pad0": 2}      # (the 1x1 hosts stay on the fp32 pipe: no X3 form)


@pytest.mark.parametrize("form,n,cin,cout,h,w,fam", [pytest.param(form, *c.values, id=form + "-" + c.id) for form, ks in TAIL_KS.items() for c in fam_cases(TAIL_SHAPES, ks)])
def test_tail_backward_epilogue_with_res2_and_pool(form, n, cin, cout, h, w, fam):
    """CTL_EPI_TAILBWD: y = g = dOut * leaky'(out), partials (sum g, sum g*v); the 1x1 hosts also write the 2x2 sum-pool of g where
    ctl_conv_pool_ok says the tile configuration can"""
    ks = TAIL_KS[form]
    fams = need(fam, cin, cout, ks)
    g = gen_for(n, cin, cout, h, w, 10 + ks)
    groups = 2 if n % 2 == 0 else 1
    gi = group_index(n, groups)
    out0, v0 = torch.randn(n, cout, h, w, generator=g), torch.randn(n, cout, h, w, generator=g)
    phase = form == "phase_pad0"
    hin, win = (h // 2, w // 2) if phase else {1: (h, w), 2: (2 * h, 2 * w), 3: (h // 2, w // 2)}[ks]
    x0 = torch.randn(n, cin, hin, win, generator=g)
    wt = torch.randn(*((cin, cout, 3, 3) if phase else (cout, cin, ks, ks)), generator=g) * 0.3
    y00 = torch.randn(n, cout, h, w, generator=g)
    res = {}
    for f in each_family(fams, fam):
        b16 = f == "bf16"
        dt, x16, y16, r16 = fam_dt(f, cin, cout)
        q = rb if b16 else f64
        rnd = (lambda t: t.to(torch.bfloat16).float()) if b16 else (lambda t: t)
        out, v, x, y0 = rnd(out0), rnd(v0), rnd(x0), rnd(y00)
        flags = _ffi.EPI_TAILBWD | _ffi.EPI_STATS | (_ffi.EPI_ACCUM if form == "1x1_accum" else 0)
        if phase:      # the four phase problems of a stride-2 3x3 data gradient write dOut: weights [cin][cout][3][3] of the forward conv
            kw = dict(n=n, hin=h // 2, win=w // 2, cin=cin, hout=h // 2, wout=w // 2, cout=cout, ks=2, stride=1, pad=0, nsub=4, out_h=h, out_w=w, out_sy=2,
                      out_sx=2, out_sub=1, groups=groups, epi_slope=SLOPE, dt=dt, epi_flags=flags)
            ref = F.conv_transpose2d(q(x), q(wt), stride=2, padding=1, output_padding=1)
        elif ks == 1:
            kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=1, pad=0, groups=groups, epi_slope=SLOPE, dt=dt, epi_flags=flags)
            ref = F.conv2d(q(x), q(wt)) + (y0.double() if form == "1x1_accum" else 0.0)
        elif ks == 2:
            kw = dict(n=n, hin=2 * h, win=2 * w, cin=cin, hout=h, wout=w, cout=cout, ks=2, stride=2, pad=0, groups=groups, epi_slope=SLOPE, dt=dt, epi_flags=flags)
            ref = F.conv2d(q(x), q(wt), stride=2)
        else:
            kw = dict(n=n, hin=h // 2, win=w // 2, cin=cin, hout=h, wout=w, cout=cout, ks=3, in_mode=_ffi.IN_ZINS2, groups=groups, epi_slope=SLOPE, dt=dt,
                      epi_flags=flags)
            xz = torch.zeros(n, cin, h, w, dtype=torch.float64)
            xz[:, :, ::2, ::2] = q(x)
            ref = F.conv2d(xz, q(wt), padding=1)
        pool_shape = (n, cout, h // 2, w // 2) if ks == 1 and lib.ctl_conv_pool_ok(_ffi.desc_ptr(_ffi.conv_desc(**kw))) else None
        if ks == 1:
            assert ((n, cin, cout, h, w) in POOL_SHAPES) == (pool_shape is not None), "ctl_conv_pool_ok: the pool path is taken at exactly the POOL_SHAPES"
        wp = pack_phases(f, wt, cout, cin, (9, cout * 9, 3, 1), 3) if phase else pack_fwd(f, wt)
        o = run_conv(kw, dev(x, x16), wp, (n, cout, h, w), y16, y_init=y0 if form == "1x1_accum" else None, want_stats=True,
                     pool_shape=pool_shape, res=dev(out, r16), res2=dev(v, r16))
        gref = ref * torch.where(out > 0, 1.0, SLOPE).double()
        what = f"{f} tail epilogue {form}"
        judge(f, o["y"], gref, what, b16out=y16, got32=res.get("y"))
        if pool_shape is not None:
            judge(f, o["pool"], F.avg_pool2d(gref, 2) * 4.0, what + " pool", b16out=y16, got32=res.get("pool"))
        part = o["stats"].sum(1)
        assert bool(torch.isfinite(part).all()), what + ": non-finite partial sums"
        for k in range(groups):                                # the rule of test_tail_backward_epilogue
            sel = gi == k
            r0, r1 = gref[sel].sum((0, 2, 3)), (gref[sel] * v[sel].double()).sum((0, 2, 3))
            assert float((part[k, 0] - r0).abs().max()) <= 5e-4 * float(gref[sel].abs().sum((0, 2, 3)).max()) + 1e-3, what + " sum g"
            assert float((part[k, 1] - r1).abs().max()) <= 5e-4 * float((gref[sel] * v[sel].double()).abs().sum((0, 2, 3)).max()) + 1e-3, what + " sum g*v"
        if f == "fp32":
            res["y"], res["pool"] = o["y"], o.get("pool")


# ------------------------------------------------------------------------------------------------ the channel-pad lanes read nothing
@pytest.mark.parametrize("n,cin,cout,h,w,fam", fam_cases(OFFGRID[:4] + OFFGRID[-2:] + OFFGRID_TILED[:1] + NARROW[1:2], 3, ["fp32", "bf16"]))
def test_a_poisoned_pixel_reaches_exactly_its_receptive_field(n, cin, cout, h, w, fam):
    """cin 4 / 8 / 12: the staging pads a pixel's channels to 16 lanes, and in NHWC the lanes past cin are the NEXT pixel's channels.  A
    channel mask that lets one quad too many through multiplies real, finite data by the pack's zero rows: invisible in every comparison
    above.  With one pixel of x set to NaN it is not: the NaN must arrive in the 3x3 neighbourhood of that pixel and nowhere else, while a
    quad read across the pixel boundary carries it (0 * NaN) into the outputs around the pixel BEFORE it in memory -- the left neighbour,
    or, for the first pixel of a row, the last pixel of the row above.  Everything else is held to the reference by the family's rule."""
    g = gen_for(n, cin, cout, h, w, 77)
    x0 = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2 + 0.05      # (no weight is 0: every output channel of the neighbourhood sees the NaN)
    dt, x16, y16, _ = fam_dt(fam, cin, cout)
    assert not x16
    q = rb if fam == "bf16" else f64
    wp = pack_fwd(fam, wt)
    ref = F.conv2d(q(x0), q(wt), padding=1)
    for h0, w0 in [(h // 2, w // 2), (h // 2, 0), (h - 1, w - 1)]:
        x = x0.clone()
        x[0, :, h0, w0] = float("nan")
        kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3, dt=dt)
        got = run_conv(kw, dev(x), wp, (n, cout, h, w), y16)["y"].float()
        hit = torch.zeros(n, 1, h, w, dtype=torch.bool)
        hit[0, 0, max(h0 - 1, 0):h0 + 2, max(w0 - 1, 0):w0 + 2] = True
        hit = hit.expand(n, cout, h, w)
        what = f"{fam} conv3x3 with x[0, :, {h0}, {w0}] = NaN"
        assert bool(torch.isnan(got[hit]).all()), f"{what}: an output of the pixel's 3x3 neighbourhood did not see it"
        stray = torch.nonzero(~torch.isfinite(got) & ~hit)
        assert stray.numel() == 0, f"{what}: {stray.shape[0]} outputs outside its receptive field are not finite, first (n, c, h, w) = {stray[0].tolist()}"
        if fam == "bf16":
            judge(fam, torch.where(hit, ref.float(), got), ref, what, b16out=y16)
        else:
            judge(fam, torch.where(hit, ref.float(), got), ref, what)


# ------------------------------------------------------------------------------------------------ forms with no off-grid variant
REFUSED_FORMS = {      # form -> (families, the OFFGRID shapes it is refused for)
    "bn_backward_prologue": (("fp32", "bf16"), lambda cin, cout: cin % 16 != 0),
    "tail_epilogue": (("fp32", "bf16"), lambda cin, cout: cout % 16 != 0),
    "bnbwd_epilogue": (("bf16",), lambda cin, cout: cin % 16 != 0 or cout % 16 != 0),
    "x3": (("x3",), lambda cin, cout: not x3_ok(cin, cout, 3)),
}


@pytest.mark.parametrize("form,n,cin,cout,h,w,fam", [pytest.param(form, *s, f, id=f"{form}-" + "-".join(map(str, s)) + f"-{f}")
                                                     for form, (fams, bad) in REFUSED_FORMS.items() for s in OFFGRID for f in fams if bad(s[1], s[2])])
def test_offgrid_forms_are_refused_by_name(form, n, cin, cout, h, w, fam):
    """The fused backward forms are built on whole 16-channel tiles (the prologue's coefficient quads, the epilogues' row reductions), and
    the X3 family on whole cin chunks: at an off-grid channel count the call returns an error that names the count and writes nothing.
    nets.py keeps these layers on the unfused passes instead (tests/test_config_contract_cpu.py)."""
    dt = _ffi.DT_X3 if fam == "x3" else fam_dt(fam, cin, cout)[0]
    kw = dict(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3, dt=dt)
    if form == "bn_backward_prologue":
        refused(dict(kw, pro_affine=2, epi_flags=_ffi.EPI_STATS), [f"cin {cin}"])
    elif form == "tail_epilogue":
        refused(dict(kw, ks=1, pad=0, epi_flags=_ffi.EPI_TAILBWD | _ffi.EPI_STATS, epi_slope=SLOPE), [f"cout {cout}"])
    elif form == "bnbwd_epilogue":
        refused(dict(kw, epi_flags=_ffi.EPI_BNBWD | _ffi.EPI_STATS, epi_slope=SLOPE), [f"cin {cin}", f"cout {cout}"])
    else:
        refused(kw, [f"cin {cin}, cout {cout}"])


# ------------------------------------------------------------------------------------------------ the checks bite on the device too
@pytest.mark.parametrize("which", ["y", "stats_partial"])
def test_a_payload_one_row_short_is_reported_as_exactly_the_missing_bytes(which):
    """The payload is declared one row (cout floats) shorter than the tensor shape / ctl_conv_stats_floats says.  The kernel writes its
    last row into the back guard of the test's own allocation (256 KiB; nothing faults), and check_guards reports exactly those bytes."""
    n, cin, cout, h, w = 2, 16, 16, 9, 7
    g = gen_for(n, cin, cout, h, w, 99)
    x = dev(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    b = dev(torch.randn(cout, generator=g) + 3.0)              # (no output is an exact zero or carries the guard's byte pattern)
    d = _ffi.conv_desc(n=n, hin=h, win=w, cin=cin, hout=h, wout=w, cout=cout, ks=3, epi_flags=_ffi.EPI_BIAS | _ffi.EPI_STATS)
    dp = _ffi.desc_ptr(d)
    ny, ns = n * h * w * cout, int(lib.ctl_conv_stats_floats(dp))
    y = Guarded(ny - (cout if which == "y" else 0), torch.float32, DEV, name="y")
    st = Guarded(ns - (cout if which == "stats_partial" else 0), torch.float32, DEV, name="stats_partial")
    wp = pack_fwd("fp32", wt)
    check(lib.ctl_conv_forward_ex(dp, x.data_ptr(), wp.data_ptr(), b.data_ptr(), None, None, None, None, None, None, None, y.ptr, st.ptr, None, None,
                                  ops.stream_ptr()))
    short, whole = (y, st) if which == "y" else (st, y)
    whole.check_guards()
    whole.check_written()
    short.check_written()
    v = short.guard_violations()
    row = short._back()[:4 * cout].cpu()
    # exactly the missing row: all of its floats were written (none still is guard pattern), nothing beyond it was; a byte of a written
    # float that happens to equal the pattern's 0x5A cannot count as touched, so the expected count is taken from the row itself
    assert bool((row.view(torch.int32) != 0x5A5A5A5A).all()), "a float of the missing row was not written"
    same = int((row == 0x5A).sum())
    assert len(v) == 1 and v[0]["side"] == "back" and short.nbytes <= v[0]["first"] and v[0]["last"] < short.nbytes + 4 * cout, v
    assert v[0]["count"] == 4 * cout - same, (v, same)
    ref = F.conv2d(x.cpu().double(), wt.double(), b.cpu().double(), padding=1)
    if which == "y":
        got = row.view(torch.float32).double()
        assert float((got - ref[-1, :, -1, -1]).abs().max()) <= 2e-4 * float(ref.abs().max()), "the guard holds the last pixel's channels"
    with pytest.raises(AssertionError):
        short.check_guards()
