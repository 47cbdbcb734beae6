"""The vector-tail kernels of csrc/ctl_elem.hip behind guard bands (oracle/guarded.py).  These kernels move quads (16 bytes of fp32) or
octets (16 bytes of bf16) per lane and round their grids up; production hands them arena tensors packed at 256-byte granularity, so a tail
lane that stores one vector too many writes into the neighbouring tensor.  Every output here is a Guarded payload of exactly the tensor's
bytes, poisoned; after the call the guards must be intact and every element written, the values are held to oracle/ref_elem.py at the
tolerances of tests/test_elem_gpu.py, and a second run over re-poisoned outputs must give the same bits.

(pixels, c) and the counts are the smallest with a partial last vector, a partial last block and more than one block."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check  # noqa: E402
from oracle import ref_elem as R  # noqa: E402
from oracle.guarded import GuardedCall  # noqa: E402

DEV = "cuda"
F64 = torch.float64
SLOPE, EPS, MOM = 0.2, 1e-5, 0.1
U24 = 2.0 ** -24
WIDE = [(63, 16), (9 * 7 * 3, 32), (5, 128), (1, 16)]           # (pixels, c) with c >= 16: the BatchNorm element-wise kernels
ROWS = [(4097, 4), (333, 3), (77, 7)]                        # c <= 7: the per-pixel row kernels
COUNTS = [1, 3, 1023, 4099]
BF = torch.bfloat16


def sp():
    return ops.stream_ptr()


def q(t, b16):
    """values exact in the storage type, as float64"""
    return R.rb(t) if b16 else t.float().double()


def put(t, b16=False):
    """[1, c, pixels, 1] reference values -> device rows [pixels][c] in the storage type"""
    t = t.to(BF if b16 else torch.float32).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def vec(t):
    return t.to(torch.float32).to(DEV).contiguous()


def nchw(buf, c, pixels):
    """Guarded rows [pixels][c] -> CPU float64 [1, c, pixels, 1]"""
    return buf.flat().view(pixels, c).t().reshape(1, c, pixels, 1).cpu().double()


def draw(pixels, c, g, lo=0.5):
    """like-signed values, so that per-channel sums are definite (see tests/test_elem_gpu.py::_definite)"""
    return torch.rand(1, c, pixels, 1, generator=g, dtype=F64) + lo


# ================================================================================================ BatchNorm element-wise chain
@pytest.mark.parametrize("b16", [0, 1])
@pytest.mark.parametrize("pixels,c", WIDE)
def test_bn_act_dt(pixels, c, b16):
    g = torch.Generator().manual_seed(pixels + c)
    x = q(torch.randn(1, c, pixels, 1, generator=g, dtype=F64), b16)
    sc, sh = q(torch.rand(1, c, generator=g, dtype=F64) + 0.5, 0), q(torch.randn(1, c, generator=g, dtype=F64) * 0.5, 0)
    xd, scd, shd = put(x, b16), vec(sc), vec(sh)
    ref = R.bn_act(x, sc, sh, SLOPE, 1)
    for y16 in (0, 1):
        gc = GuardedCall(DEV)
        y = gc.out("y", pixels * c, BF if y16 else torch.float32)
        launch = lambda: check(lib.ctl_bn_act_dt(xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), SLOPE, y.ptr, pixels, c, 1, b16 | y16 << 1, sp()))
        gc.run(launch)
        R.close(nchw(y, c, pixels), ref, 1e-5, f"bn_act x16={b16} y16={y16}", bf16_out=bool(y16))
        gc.rerun(launch)
    if not b16:
        gc = GuardedCall(DEV)
        y = gc.out("y", pixels * c)
        launch = lambda: check(lib.ctl_bn_act(xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), SLOPE, y.ptr, pixels, c, 1, sp()))
        gc.run(launch)
        R.close(nchw(y, c, pixels), ref, 1e-5, "bn_act")
        gc.rerun(launch)


@pytest.mark.parametrize("b16", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("pixels,c", WIDE)
def test_bwd_reduce_dt_partials_and_ds(pixels, c, mode, b16):
    """the partial buffer is exactly ctl_bwd_reduce_rows rows of [2][c]; every row is read by the finalize kernels, so every row must be
    written (a grid of `rows` blocks over a handful of quads: the blocks without work still own their row)"""
    g = torch.Generator().manual_seed(pixels + c + mode)
    dy, act, u = q(draw(pixels, c, g), b16), q(draw(pixels, c, g) - 1.0, b16), q(-draw(pixels, c, g), b16)
    sc, sh = q(torch.rand(1, c, generator=g, dtype=F64) + 0.5, 0), torch.zeros(1, c, dtype=F64)
    dyd, actd, ud, scd, shd = put(dy, b16), put(act, b16), put(u, b16), vec(sc), vec(sh)
    rows = int(lib.ctl_bwd_reduce_rows(mode, pixels, c))
    gref = R.bwd_g(mode, dy, act_src=act, u=u, scale=sc, shift=sh, slope=SLOPE, groups=1)
    s1, s2 = R.bwd_sums(gref, u, 1)
    for with_ds in ((0, 1) if mode == 0 else (0,)):
        gc = GuardedCall(DEV)
        part = gc.out("partial", rows * 2 * c)
        ds = gc.out("ds", pixels * c, BF if b16 else torch.float32) if with_ds else None
        mask = ((1 if mode == 2 else 7) if b16 else 0) | ((8 if b16 else 0) if with_ds else 0)

        def launch():
            check(lib.ctl_bwd_reduce_dt(mode, dyd.data_ptr(), actd.data_ptr() if mode == 0 else None, ud.data_ptr() if mode < 2 else None,
                                        scd.data_ptr() if mode == 1 else None, shd.data_ptr() if mode == 1 else None, SLOPE, pixels, c, part.ptr, 1, mask,
                                        ds.ptr if with_ds else None, sp()))

        gc.run(launch)
        sums = part.flat().cpu().double().view(rows, 2, c).sum(0)
        R.close(sums[0].view(1, c), s1, 2e-4, f"sum g (mode {mode}, ds {with_ds})", per_channel=True)
        if mode < 2:
            R.close(sums[1].view(1, c), s2, 2e-4, f"sum g*u (mode {mode}, ds {with_ds})", per_channel=True)
        if with_ds:
            R.close(nchw(ds, c, pixels), gref, 1e-5, "ds of the reduce pass", per_channel=True, bf16_out=bool(b16))
        gc.rerun(launch)
    if not b16:                                                 # the plain entry point, and its consumer ctl_chan_sum_finalize for mode 2
        gc = GuardedCall(DEV)
        part = gc.out("partial", rows * 2 * c)
        out = gc.out("out", c) if mode == 2 else None

        def launch32():
            check(lib.ctl_bwd_reduce(mode, dyd.data_ptr(), actd.data_ptr() if mode == 0 else None, ud.data_ptr() if mode < 2 else None,
                                     scd.data_ptr() if mode == 1 else None, shd.data_ptr() if mode == 1 else None, SLOPE, pixels, c, part.ptr, 1, sp()))
            if mode == 2:
                check(lib.ctl_chan_sum_finalize(part.ptr, c, out.ptr, 0, sp()))

        gc.run(launch32)
        R.close(part.flat().cpu().double().view(rows, 2, c).sum(0)[0].view(1, c), s1, 2e-4, "sum g, plain entry", per_channel=True)
        if mode == 2:
            R.close(out.flat().cpu().double().view(1, c), s1, 2e-4, "channel sums", per_channel=True)
        gc.rerun(launch32)


@pytest.mark.parametrize("b16", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("pixels,c", WIDE)
def test_bwd_apply_dt_dx_and_ds(pixels, c, mode, b16):
    g = torch.Generator().manual_seed(pixels + c + mode + 11)
    sign = torch.where(torch.rand(1, c, pixels, 1, generator=g, dtype=F64) < 0.5, -1.0, 1.0).to(F64)
    dy, act = q(torch.randn(1, c, pixels, 1, generator=g, dtype=F64), b16), q(draw(pixels, c, g) * sign, b16)
    u = q(draw(pixels, c, g) * sign, b16)                       # |u * scale| >= 0.25: the slope choice of mode 1 is never a rounding matter
    sc, sh = q(torch.rand(1, c, generator=g, dtype=F64) + 0.5, 0), torch.zeros(1, c, dtype=F64)
    coef = q(torch.randn(1, 3, c, generator=g, dtype=F64), 0)
    dyd, actd, ud, scd, shd, cfd = put(dy, b16), put(act, b16), put(u, b16), vec(sc), vec(sh), vec(coef)
    gref = R.bwd_g(mode, dy, act_src=act, u=u, scale=sc, shift=sh, slope=SLOPE, groups=1)
    ref = R.bwd_apply(gref, u, coef[:, 0], coef[:, 1], coef[:, 2], 1)
    for with_ds in ((0, 1) if mode == 0 else (0,)):
        gc = GuardedCall(DEV)
        dx = gc.out("dx", pixels * c, BF if b16 else torch.float32)
        ds = gc.out("ds", pixels * c, BF if b16 else torch.float32) if with_ds else None
        mask = (1 | 2 | 4 | 16 | (8 if with_ds else 0)) if b16 else 0

        def launch():
            check(lib.ctl_bwd_apply_dt(mode, dyd.data_ptr(), actd.data_ptr() if mode == 0 else None, ud.data_ptr(), scd.data_ptr() if mode == 1 else None,
                                       shd.data_ptr() if mode == 1 else None, SLOPE, cfd.data_ptr(), pixels, c, ds.ptr if with_ds else None, dx.ptr, 1, mask, sp()))

        gc.run(launch)
        R.close(nchw(dx, c, pixels), ref, 1e-5, f"dx (mode {mode}, ds {with_ds})", bf16_out=bool(b16))
        if with_ds:
            R.close(nchw(ds, c, pixels), gref, 1e-5, "ds of the apply pass", bf16_out=bool(b16))
        gc.rerun(launch)
    if not b16:
        gc = GuardedCall(DEV)
        dx = gc.out("dx", pixels * c)
        launch32 = lambda: check(lib.ctl_bwd_apply(mode, dyd.data_ptr(), actd.data_ptr() if mode == 0 else None, ud.data_ptr(), scd.data_ptr() if mode == 1 else None,
                                                   shd.data_ptr() if mode == 1 else None, SLOPE, cfd.data_ptr(), pixels, c, None, dx.ptr, 1, sp()))
        gc.run(launch32)
        R.close(nchw(dx, c, pixels), ref, 1e-5, f"dx, plain entry (mode {mode})")
        gc.rerun(launch32)


@pytest.mark.parametrize("n,c,h,w", [(3, 16, 5, 7), (1, 4, 1, 1), (2, 128, 3, 1), (2, 8, 7, 9)])
def test_sumpool2_odd_pooled_sizes(n, c, h, w):
    """(h, w) is the pooled size; additions only, so the fp32 association (a0 + a1) + (a2 + a3) is exact to compare"""
    g = torch.Generator().manual_seed(c + h)
    up = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    prev = torch.randn(n, c, h, w, generator=g)
    pool32 = lambda x: (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])
    for in16 in (0, 1):
        upv = up.to(BF).float() if in16 else up
        upd = put(upv, in16)
        for out16 in ((0, 1) if in16 else (0,)):
            for acc in (0, 1):
                pv = prev.to(BF).float() if out16 else prev
                pd = put(pv, out16)
                gc = GuardedCall(DEV)
                dx = gc.out("dx", n * c * h * w, BF if out16 else torch.float32,
                            init=(lambda b: b.view((n, c, h, w), channels_last=True).copy_(pd)) if acc else None)

                def launch():
                    if in16 or out16:
                        check(lib.ctl_sumpool2_dt(upd.data_ptr(), dx.ptr, n, h, w, c, acc, in16 | out16 << 1, sp()))
                    else:
                        check(lib.ctl_sumpool2(upd.data_ptr(), dx.ptr, n, h, w, c, acc, sp()))

                gc.run(launch)
                want = pool32(upv) + (pv if acc else 0.0)
                got = dx.view((n, c, h, w), channels_last=True).cpu()
                assert torch.equal(got.float(), want.to(BF).float() if out16 else want), f"sum-pool in16={in16} out16={out16} accumulate={acc}"
                R.close(got.double(), R.sumpool2(upv) + (pv.double() if acc else 0.0), 1e-6, "sum-pool against float64", bf16_out=bool(out16))
                gc.rerun(launch)


# ================================================================================================ flat streams
@pytest.mark.parametrize("count", COUNTS)
def test_flat_stream_kernels(count):
    """ctl_chan_sum_finalize, ctl_sigmoid_bwd, ctl_accumulate, ctl_mse_fwd / ctl_mse_bwd and ctl_adam on `count` elements"""
    g = torch.Generator().manual_seed(count)
    # channel sums of a hand-made [CTL_RED_BLOCKS][2][c] partial buffer (row 1 is not this kernel's business: NaN)
    c, rb_ = count, int(lib.ctl_red_blocks())
    part = torch.rand(rb_, 2, c, generator=g) + 0.5
    part[:, 1] = float("nan")
    partd = part.to(DEV)
    prev = torch.rand(c, generator=g)
    for acc in (0, 1):
        gc = GuardedCall(DEV)
        out = gc.out("out", c, init=(lambda b: b.flat().copy_(prev.to(DEV))) if acc else None)
        launch = lambda: check(lib.ctl_chan_sum_finalize(partd.data_ptr(), c, out.ptr, acc, sp()))
        gc.run(launch)
        R.close(out.flat().cpu().double().view(1, c), (part[:, 0].double().sum(0) + (prev.double() if acc else 0.0)).view(1, c), 2e-4,
                f"channel sums accumulate={acc}", per_channel=True)
        gc.rerun(launch)
    # sigmoid backward
    y = torch.sigmoid(torch.randn(count, generator=g) * 4)
    dy = torch.randn(count, generator=g)
    yd, dyd = y.to(DEV), dy.to(DEV)
    gc = GuardedCall(DEV)
    dx = gc.out("dx", count)
    launch = lambda: check(lib.ctl_sigmoid_bwd(dyd.data_ptr(), yd.data_ptr(), dx.ptr, count, sp()))
    gc.run(launch)
    R.close(dx.flat(), R.sigmoid_bwd(dy, y), 1e-6, "sigmoid backward")
    gc.rerun(launch)
    # k-way accumulate: the ordered fp32 sum, exact
    for k in (1, 3, 8):
        dst0 = torch.randn(count, generator=g)
        srcs = [torch.randn(count, generator=g) for _ in range(k)]
        sd = [s.to(DEV) for s in srcs]
        arr = (ctypes.c_void_p * k)(*[s.data_ptr() for s in sd])
        gc = GuardedCall(DEV)
        dst = gc.out("dst", count, init=lambda b: b.flat().copy_(dst0.to(DEV)))
        launch = lambda: check(lib.ctl_accumulate(dst.ptr, arr, k, count, sp()))
        gc.run(launch)
        ref = dst0.clone()
        for s in srcs:
            ref = ref + s
        assert torch.equal(dst.flat().cpu(), ref), f"accumulate k={k}"
        gc.rerun(launch)
    # mse
    a, b = torch.rand(count, generator=g), torch.rand(count, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    gout = torch.tensor(0.7, device=DEV)
    gc = GuardedCall(DEV)
    mpart = gc.out("partial", rb_, F64, written=False)         # (the finalize launch reads the blocks the partial launch ran)
    loss = gc.out("loss", 1)
    da = gc.out("da", count)

    def launch():
        check(lib.ctl_mse_fwd(ad.data_ptr(), bd.data_ptr(), count, 0.5, mpart.ptr, loss.ptr, sp()))
        check(lib.ctl_mse_bwd(ad.data_ptr(), bd.data_ptr(), gout.data_ptr(), count, 0.5, da.ptr, sp()))

    gc.run(launch)
    ref = R.mse(a, b, 0.5)
    assert abs(float(loss.flat()[0]) - ref) <= 4 * U24 * ref + 1e-45, (float(loss.flat()[0]), ref)
    R.close(da.flat(), R.mse_grad(a, b, float(np.float32(0.7)), 0.5), 1e-5, "mse backward")
    gc.rerun(launch)
    # Adam, in place on three guarded tensors
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-8
    p0, gr = torch.randn(count, generator=g), torch.randn(count, generator=g) * 0.1
    m0, v0 = gr * 0.05, gr * gr * 0.001
    grd = gr.to(DEV)
    gc = GuardedCall(DEV)
    pb = gc.out("p", count, init=lambda t: t.flat().copy_(p0.to(DEV)))
    mb = gc.out("m", count, init=lambda t: t.flat().copy_(m0.to(DEV)))
    vb = gc.out("v", count, init=lambda t: t.flat().copy_(v0.to(DEV)))
    launch = lambda: check(lib.ctl_adam(pb.ptr, grd.data_ptr(), mb.ptr, vb.ptr, count, lr, b1, b2, eps, 3, 1.0, sp()))
    gc.run(launch)
    pr, mr, vr = R.adam(p0, gr, m0, v0, *(float(np.float32(t)) for t in (lr, b1, b2, eps)), 3, 1.0)
    assert bool(((pb.flat().cpu().double() - pr).abs() <= 2e-7 * pr.abs().clamp_min(1.0)).all()), "adam p"
    for name, got, want in (("m", mb, mr), ("v", vb, vr)):
        tol = torch.where(want.abs() < 2.0 ** -126, torch.full_like(want, 2.0 ** -126), 4 * U24 * want.abs())      # the rule of tests/test_elem_gpu.py
        assert bool(((got.flat().cpu().double() - want).abs() <= tol).all()), f"adam {name}"
    gc.rerun(launch)


# ================================================================================================ BatchNorm finalize kernels
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("c", [16, 3, 130])
def test_bn_finalize_ex_bwd_finalize_ex_and_eval_coeffs(c, groups):
    """every coefficient vector is [groups][c] (coef: [groups][3][c]); hand-made partial rows with definite (like-signed) sums"""
    g = torch.Generator().manual_seed(c + groups)
    blocks, count = 5, 77
    x = torch.randn(groups, count, c, generator=g, dtype=F64) * 0.7 + 2.0
    per_block = [x[:, i::blocks] for i in range(blocks)]
    part = torch.stack([torch.stack([pb.sum(1), (pb ** 2).sum(1)], 1) for pb in per_block], 1).float()      # [groups][blocks][2][c]
    gamma, beta = q(torch.rand(c, generator=g, dtype=F64) + 0.5, 0), q(-(torch.rand(c, generator=g, dtype=F64) + 0.5), 0)
    rm, rv = q(torch.rand(c, generator=g, dtype=F64) + 1.0, 0), q(torch.rand(c, generator=g, dtype=F64) + 0.5, 0)
    partd, gd, bd = part.to(DEV).contiguous(), vec(gamma), vec(beta)
    s1, s2 = part.double()[:, :, 0].sum(1), part.double()[:, :, 1].sum(1)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    invstd = 1 / torch.sqrt(var + EPS)
    want = dict(scale=gamma * invstd, shift=beta - mean * gamma * invstd, mean=mean, invstd=invstd, uvar=var * count / (count - 1))
    gc = GuardedCall(DEV)
    outs = {k: gc.out(k, groups * c) for k in ("scale", "shift", "mean", "invstd", "uvar")}
    rmb = gc.out("running_mean", c, init=lambda t: t.flat().copy_(vec(rm)))
    rvb = gc.out("running_var", c, init=lambda t: t.flat().copy_(vec(rv)))
    nbt = gc.out("num_batches_tracked", 1, torch.int64, init=lambda t: t.flat().fill_(5))

    def launch():
        check(lib.ctl_bn_finalize_ex(partd.data_ptr(), blocks, c, count, gd.data_ptr(), bd.data_ptr(), EPS, MOM, 1, rmb.ptr, rvb.ptr, nbt.ptr,
                                     outs["scale"].ptr, outs["shift"].ptr, outs["mean"].ptr, outs["invstd"].ptr, outs["uvar"].ptr, groups, sp()))

    gc.run(launch)
    for k, b in outs.items():
        R.close(b.flat().cpu().double().view(groups, c), want[k], 1e-5, k, per_channel=True)
    rme, rve = rm.clone(), rv.clone()
    for k in range(groups):
        rme, rve = (1 - MOM) * rme + MOM * want["mean"][k], (1 - MOM) * rve + MOM * want["uvar"][k]
    R.close(rmb.flat().cpu().double().view(1, c), rme.view(1, c), 1e-5, "running_mean", per_channel=True)
    R.close(rvb.flat().cpu().double().view(1, c), rve.view(1, c), 1e-5, "running_var", per_channel=True)
    assert int(nbt.flat()[0]) == 5 + groups
    gc.rerun(launch)
    # backward finalize: partial rows (sum g, sum g*u) -> coef [groups][3][c], dgamma / dbeta
    gsum = torch.rand(groups, blocks, 2, c, generator=g, dtype=F64) + 0.5
    gsum[:, :, 1] *= -1.0
    gpart = gsum.float().to(DEV).contiguous()
    md, isd = vec(torch.rand(groups, c, generator=g, dtype=F64) + 0.5), vec(torch.rand(groups, c, generator=g, dtype=F64) + 0.5)
    A, B, C, sum_g, sum_gx = R.bwd_coefs(gsum.float().double()[:, :, 0].sum(1), gsum.float().double()[:, :, 1].sum(1), count, gamma, R.f64(md).view(groups, c),
                                         R.f64(isd).view(groups, c))
    dg0, db0 = q(torch.rand(c, generator=g, dtype=F64), 0), q(torch.rand(c, generator=g, dtype=F64), 0)
    for acc in (0, 1):
        gc = GuardedCall(DEV)
        coef = gc.out("coef", groups * 3 * c)
        dgam = gc.out("dgamma", c, init=(lambda t: t.flat().copy_(vec(dg0))) if acc else None)
        dbet = gc.out("dbeta", c, init=(lambda t: t.flat().copy_(vec(db0))) if acc else None)
        launch = lambda: check(lib.ctl_bn_bwd_finalize_ex(gpart.data_ptr(), c, count, gd.data_ptr(), md.data_ptr(), isd.data_ptr(), coef.ptr, dgam.ptr, dbet.ptr,
                                                          acc, groups, blocks, 0, sp()))
        gc.run(launch)
        cf = coef.flat().cpu().double().view(groups, 3, c)
        for k, (name, ref) in enumerate((("A", A), ("B", B), ("C", C))):
            R.close(cf[:, k], ref, 5e-4, f"{name} (accumulate {acc})", per_channel=True)
        dg_ref, db_ref = R.bwd_dparams(sum_g, sum_gx, dg0, db0, bool(acc), 0)
        R.close(dgam.flat().cpu().double().view(1, c), dg_ref.view(1, c), 5e-4, f"dgamma (accumulate {acc})", per_channel=True)
        R.close(dbet.flat().cpu().double().view(1, c), db_ref.view(1, c), 5e-4, f"dbeta (accumulate {acc})", per_channel=True)
        gc.rerun(launch)
    # inference-mode coefficients
    rmd, rvd = vec(rm), vec(rv)
    gc = GuardedCall(DEV)
    scale, shift = gc.out("scale", groups * c), gc.out("shift", groups * c)
    launch = lambda: check(lib.ctl_bn_eval_coeffs(c, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), EPS, scale.ptr, shift.ptr, groups, sp()))
    gc.run(launch)
    sc, sh = R.bn_eval_coeffs(gamma, beta, rm, rv, EPS, groups)
    R.close(scale.flat().cpu().double().view(groups, c), sc, 1e-6, "eval scale", per_channel=True)
    R.close(shift.flat().cpu().double().view(groups, c), sh, 1e-6, "eval shift", per_channel=True)
    gc.rerun(launch)


# ================================================================================================ per-pixel row kernels
@pytest.mark.parametrize("pixels,c", ROWS)
def test_softmax_onehot_argmax_cross_entropy_rows(pixels, c):
    g = torch.Generator().manual_seed(pixels + c)
    x = torch.randn(pixels, c, generator=g) * 3
    dp = torch.randn(pixels, c, generator=g)
    lab = torch.randint(0, c, (pixels,), generator=g)
    xd, dpd, labd = x.to(DEV), dp.to(DEV), lab.to(DEV)
    gout = torch.tensor(0.7, device=DEV)
    rows = lambda t: t.t().reshape(1, c, pixels, 1)
    xr = rows(x.double())
    gc = GuardedCall(DEV)
    p, dx, oh, dl = (gc.out(k, pixels * c) for k in ("p", "dx", "onehot", "dlogit"))
    am = gc.out("argmax", pixels, torch.uint8, written=False)   # (class 90 = 0x5A cannot occur with c <= 7, but the check is on bits: guards only)
    part = gc.out("partial", int(lib.ctl_red_blocks()), F64, written=False)
    loss = gc.out("loss", 1)

    def launch():
        check(lib.ctl_softmax_t_fwd(xd.data_ptr(), 0.5, p.ptr, pixels, c, sp()))
        check(lib.ctl_softmax_t_bwd(p.ptr, dpd.data_ptr(), 0.5, dx.ptr, pixels, c, sp()))
        check(lib.ctl_onehot(labd.data_ptr(), oh.ptr, pixels, c, sp()))
        check(lib.ctl_argmax_c(xd.data_ptr(), am.ptr, pixels, c, sp()))
        check(lib.ctl_ce2d_fwd(xd.data_ptr(), labd.data_ptr(), pixels, c, part.ptr, loss.ptr, sp()))
        check(lib.ctl_ce2d_bwd(xd.data_ptr(), labd.data_ptr(), gout.data_ptr(), pixels, c, dl.ptr, sp()))

    gc.run(launch)
    am.check_written()                                          # every pixel got a class < 7
    pc = p.flat().view(pixels, c).cpu().double()
    R.close(rows(pc), R.softmax_t_fwd(xr, 2.0), 1e-6, "softmax T=2")
    R.close(rows(dx.flat().view(pixels, c).cpu().double()), R.softmax_t_bwd(rows(pc), rows(dp.double()), 2.0), 1e-5, "softmax backward")
    assert torch.equal(rows(oh.flat().view(pixels, c).cpu().double()), R.onehot(lab.view(1, pixels, 1), c))
    assert torch.equal(am.flat().cpu(), R.argmax_first(xr).view(-1))
    ref = R.ce_mean(xr, lab.view(1, pixels, 1))
    assert abs(float(loss.flat()[0]) - ref) <= 2e-6 * max(1.0, abs(ref)), (float(loss.flat()[0]), ref)
    R.close(rows(dl.flat().view(pixels, c).cpu().double()), R.ce_grad(xr, lab.view(1, pixels, 1), float(np.float32(0.7))), 1e-5, "cross-entropy backward")
    gc.rerun(launch)
