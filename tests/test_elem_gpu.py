"""The HBM-bound kernels of csrc/ctl_elem.hip, each called through the C ABI and held to the plain float64 restatement of its operation
in oracle/ref_elem.py (itself checked against torch.autograd by tests/test_elem_ref_cpu.py): BatchNorm finalize / apply / backward in
every storage form, sum-pool, channel sums, the k-way accumulator, the STN input builders, the fused losses, argmax and Adam.

Inputs are exact in float64: a tensor stored as bf16 is rounded to bf16 first, an fp32 one to fp32.  Tolerances are the ones the suite
already holds these kernels to (test_kernels_gpu.py, test_bf16_gpu.py); per-channel outputs are normalised channel by channel, so a wrong
small channel cannot hide behind a large one.  Where two forms of a kernel promise the same arithmetic they are compared bit for bit.

Every negative case uses an argument the launcher refuses before it launches anything."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check, CtlError  # noqa: E402
from oracle import ref_elem as R  # noqa: E402

DEV = "cuda"
F64 = torch.float64
SLOPE, EPS, MOM = 0.2, 1e-5, 0.1
EB, MAX_STREAM_BLOCKS = 256, 2048          # block size and grid cap of the streaming kernels: one grid pass covers EB * MAX_STREAM_BLOCKS items
BIG = (16, 16, 256, 256)                   # the largest layer of the real network
U24 = 2.0 ** -24


def sp():
    return ops.stream_ptr()


def q32(t):
    return t.float().double()


def nhwc(t, b16=False):
    """CPU NCHW values -> device tensor whose memory is NHWC, stored as bf16 or fp32"""
    t = t.to(torch.bfloat16 if b16 else torch.float32).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def out_like(t, b16):
    return torch.empty_like(t, dtype=torch.bfloat16 if b16 else torch.float32)


def vec(t):
    return t.to(torch.float32).to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


# ================================================================================================ a. BatchNorm backward chain
@functools.lru_cache(maxsize=2)
def _chain_raw(shape, attempt=0):
    """Unrounded inputs of one shape.  Channels differ in magnitude by three decades.  Some layers see 9 to 32 pixels per (group, channel),
    and a per-channel relative bound on a sum of so few terms needs terms of one sign: dy > 0, u < 0 (mean / std about -2.7), dy and the
    activation sign follow xhat, so that sum g, sum g*u, sum g*xhat, C, dgamma and dbeta are definite (see _definite).  Mixed signs are
    covered by the bit-for-bit tests further down."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + c * 10 + h + w + 7919 * attempt)
    mag = 10.0 ** (torch.rand(c, generator=g, dtype=F64) * 3 - 2)
    off = torch.randn(c, generator=g, dtype=F64) * 0.3 - 4.0
    u = torch.randn(n, c, h, w, generator=g, dtype=F64) * 1.5 + off.view(1, -1, 1, 1)
    xh = (u - off.view(1, -1, 1, 1)) / 1.5
    dy = (1.0 + 0.3 * xh + 0.2 * torch.randn(n, c, h, w, generator=g, dtype=F64)).clamp_min(0.05) * mag.view(1, -1, 1, 1)
    act = xh + 0.5 * torch.randn(n, c, h, w, generator=g, dtype=F64)
    act[:, :, 0, 0] = 0.0                                              # leaky'(0) = slope
    gamma = torch.rand(c, generator=g, dtype=F64) + 0.5
    beta = torch.randn(c, generator=g, dtype=F64) * 0.2
    dg0, db0 = torch.rand(c, generator=g, dtype=F64) * mag, torch.rand(c, generator=g, dtype=F64) * mag
    return u, dy, act, gamma, beta, dg0, db0


STORAGE = {      # which tensors are stored as bf16: dy, act_src, bn_src, ds, dx
    "fp32": dict(dy=0, act=0, u=0, ds=0, dx=0),
    "bf16": dict(dy=1, act=1, u=1, ds=1, dx=1),                        # the 16-byte kernels (c % 8 == 0)
    "dx32": dict(dy=1, act=1, u=1, ds=1, dx=0),                        # quad kernels on bf16 data
    "dy32": dict(dy=0, act=1, u=1, ds=1, dx=1),
}


def _mask(st):
    return st["dy"] | st["act"] << 1 | st["u"] << 2 | st["ds"] << 3 | st["dx"] << 4


def _device_forward_stats(ud32, gamma_d, beta_d, n, c, h, w, groups):
    """scale, shift, mean, invstd [groups * c] as the device forward finalize produces them (sums through ctl_bwd_reduce mode 0, act_src = 1)"""
    M = n * h * w
    rows = lib.ctl_bwd_reduce_rows(0, M // groups, c)
    part = torch.empty(groups * rows * 2 * c, device=DEV)
    ones = torch.ones_like(ud32)
    check(lib.ctl_bwd_reduce(0, ud32.data_ptr(), ones.data_ptr(), ud32.data_ptr(), None, None, SLOPE, M, c, part.data_ptr(), groups, sp()))
    scale, shift, mean, invstd = (torch.empty(groups * c, device=DEV) for _ in range(4))
    check(lib.ctl_bn_finalize_ex(part.data_ptr(), rows, c, M // groups, gamma_d.data_ptr(), beta_d.data_ptr(), EPS, MOM, 0, None, None, None,
                                 scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), None, groups, sp()))
    torch.cuda.synchronize()
    return scale, shift, mean, invstd


def _sign_ambiguous(u, scale, shift, groups):
    """mode 1 picks the slope from the sign of u*scale+shift evaluated in fp32.  Where the exact value and the fp32 mul + add disagree in
    sign (|value| under an fp32 ulp of its terms), either is a faithful evaluation: those elements (a handful in 16 M at most) are taken
    out of the element-wise comparison."""
    n = u.shape[0]
    z64 = u * R._bc(scale, n, groups) + R._bc(shift, n, groups)
    z32 = u.float() * R._bc(scale, n, groups).float() + R._bc(shift, n, groups).float()
    amb = (z64 > 0) != (z32 > 0)
    assert int(amb.sum()) <= 8, int(amb.sum())
    return amb


def _sum_T(per_group_pixels, c, mode=0):
    """fp32 additions behind one partial-row entry, the larger of the two kernel forms: the trips of one thread plus the threads of the
    block that hold the channel (EB / (c/4) in the quad form, twice that in the 16-byte form)"""
    cq = c // 4
    rows = lib.ctl_bwd_reduce_rows(mode, per_group_pixels, c)
    return min(per_group_pixels, -(-per_group_pixels * cq // (rows * EB)) + (2 if c % 8 == 0 else 1) * EB // cq)      # (never more terms than pixels)


def _definite(val, absval, tol, T):
    """A per-channel relative bound `tol` on a sum can only be asked where the sum is not a cancellation residue of its terms.  The partial
    rows carry at most T * 2^-24 of the sum of the absolute terms (everything after them is float64), a derived quantity combines up to four
    such sums, so the reference value must keep |value| >= 4 * T * 2^-24 / tol of its absolute terms.  This looks at the reference only;
    the tests draw their inputs again (next seed) until every checked quantity is definite in this sense."""
    return bool((val.abs() * (tol / (4 * T * U24)) >= absval).all())


def _chain_cases():
    small = [(1, 8, 3, 3), (3, 8, 5, 7), (2, 8, 3, 3), (2, 4, 6, 5), (2, 16, 8, 8), (2, 32, 9, 7), (2, 64, 6, 6), (2, 128, 4, 4), (6, 8, 5, 3),
             (3, 16, 4, 4), (2, 16, 160, 160)]
    out = []
    for mode in (0, 1):
        for st in STORAGE:
            for shp in small:
                for groups in (1, 2, 3):
                    if shp[0] % groups == 0 and not (shp[2] == 160 and groups == 3):
                        out.append(pytest.param(mode, st, shp, groups, id=f"m{mode}-{st}-{'x'.join(map(str, shp))}-g{groups}"))
    for mode, st, groups in ((0, "bf16", 1), (0, "fp32", 2), (1, "bf16", 2), (1, "fp32", 1)):
        out.append(pytest.param(mode, st, BIG, groups, id=f"m{mode}-{st}-big-g{groups}"))
    return out


def test_reduce_row_counts_cover_clamp_interior_and_cap():
    """the three regimes of the partial-row count, read from the library: the lower clamp, an interior value, the cap"""
    rb = lib.ctl_red_blocks()
    assert rb == _ffi.RED_BLOCKS
    assert lib.ctl_bwd_reduce_rows(0, 2 * 8 * 8, 16) == 16
    assert 16 < lib.ctl_bwd_reduce_rows(1, 2 * 160 * 160, 16) < rb
    assert lib.ctl_bwd_reduce_rows(0, 16 * 256 * 256, 16) == rb
    assert lib.ctl_bwd_reduce_rows(2, 9, 8) == rb


@pytest.mark.parametrize("mode,storage,shape,groups", _chain_cases())
def test_bn_backward_chain(mode, storage, shape, groups):
    """ctl_bwd_reduce_dt -> ctl_bn_bwd_finalize_ex -> ctl_bwd_apply_dt against the float64 chain: partial sums, A / B / C per group, dgamma /
    dbeta (accumulate, affine_groups, NULL), ds and dx."""
    n, c, h, w = shape
    big = shape == BIG
    M, per = n * h * w, n * h * w // groups
    st = STORAGE[storage]
    rnd = lambda t, b: R.rb(t) if b else q32(t)
    gd = bd = ud = dyd = actd = None
    rows0 = lib.ctl_bwd_reduce_rows(mode, per, c)
    variants = [(0, 0, False, 0), (1, 0, False, rows0), (0, 0, True, rows0)]      # accumulate, affine_groups, NULL dgamma / dbeta, blocks
    if groups == 2:
        variants += [(0, 0b01, False, 0), (0, 0b10, False, rows0), (1, 0b10, False, 0), (1, 0b01, False, rows0)]
    T = _sum_T(per, c, mode)
    for attempt in range(4):                                            # (the designed draw is definite at once on every shape here)
        u_raw, dy_raw, act_raw, gamma, beta, dg0, db0 = _chain_raw(shape, attempt)
        u, dy, act = rnd(u_raw, st["u"]), rnd(dy_raw, st["dy"]), rnd(act_raw, st["act"])
        gamma, beta, dg0, db0 = q32(gamma), q32(beta), q32(dg0), q32(db0)
        gd, bd = vec(gamma), vec(beta)
        ud32 = nhwc(u)
        scale_d, shift_d, mean_d, invstd_d = _device_forward_stats(ud32, gd, bd, n, c, h, w, groups)
        del ud32
        scale, shift, mean, invstd = (R.f64(t).view(groups, c) for t in (scale_d, shift_d, mean_d, invstd_d))
        # ---- reference
        g_ref = R.bwd_g(mode, dy, act_src=act, u=u, scale=scale, shift=shift, slope=SLOPE, groups=groups)
        s1, s2 = R.bwd_sums(g_ref, u, groups)
        A, B, C, sum_g, sum_gx = R.bwd_coefs(s1, s2, per, gamma, mean, invstd)
        # ---- is every per-channel quantity a definite sum?  (reference only)
        a1, a2 = R.bwd_sums(g_ref.abs(), u.abs(), groups)
        a_gx = invstd * (a2 + mean.abs() * a1)
        a_C = gamma.view(1, -1) * invstd * (a1 + invstd * a_gx * mean.abs()) / per
        ok = _definite(s1, a1, 2e-4, T) and _definite(s2, a2, 2e-4, T) and _definite(sum_gx, a_gx, 5e-4, T) and _definite(C, a_C, 5e-4, T)
        for acc, aff, null, _ in variants:
            if ok and not null:
                dg_ref, db_ref = R.bwd_dparams(sum_g, sum_gx, dg0, db0, bool(acc), aff)
                dg_abs, db_abs = R.bwd_dparams(a1, a_gx, dg0.abs(), db0.abs(), bool(acc), aff)
                ok = _definite(dg_ref, dg_abs, 5e-4, T) and _definite(db_ref, db_abs, 5e-4, T)
        if ok:
            break
    else:
        raise AssertionError("no draw with definite per-channel sums")
    ud, dyd, actd = nhwc(u, st["u"]), nhwc(dy, st["dy"]), nhwc(act, st["act"])
    amb = _sign_ambiguous(u, scale, shift, groups) if mode == 1 else None
    dx_ref = R.bwd_apply(g_ref, u, A, B, C, groups)

    # ---- reduce (mode 0: with and without the ds output; ds as fp32 next to bf16 tensors takes the quad kernel)
    rows = lib.ctl_bwd_reduce_rows(mode, per, c)
    ds_kinds = [None]
    if mode == 0:
        ds_kinds = ["same"] if big else [None, "same"] + (["fp32"] if storage == "bf16" else [])
    part = None
    for dk in ds_kinds:
        ds16 = st["ds"] if dk == "same" else 0
        part = torch.empty(groups * rows * 2 * c, device=DEV)           # exactly the rows the reduction writes
        ds_r = out_like(dyd, ds16) if dk else None
        m = (_mask(st) & 7) | (ds16 << 3)
        check(lib.ctl_bwd_reduce_dt(mode, dyd.data_ptr(), actd.data_ptr() if mode == 0 else None, ud.data_ptr(),
                                    scale_d.data_ptr() if mode == 1 else None, shift_d.data_ptr() if mode == 1 else None, SLOPE, M, c,
                                    part.data_ptr(), groups, m, ops.ptr(ds_r), sp()))
        sums = part.cpu().double().view(groups, rows, 2, c).sum(1)
        for k in range(groups):
            R.close(sums[k, 0], s1[k], 2e-4, f"sum g (group {k}, ds {dk})", per_channel=True)
            R.close(sums[k, 1], s2[k], 2e-4, f"sum g*u (group {k}, ds {dk})", per_channel=True)
        if dk:
            R.close(ds_r, g_ref, 1e-5, f"ds of the reduce pass ({dk})", per_channel=True, bf16_out=bool(ds16))

    # ---- finalize: every (accumulate, affine_groups, NULL outputs) form on the same partial rows
    coef0 = None
    for acc, aff, null, blocks in variants:
        coef = torch.full((groups * 3 * c,), float("nan"), device=DEV)
        dgam, dbet = vec(dg0), vec(db0)
        check(lib.ctl_bn_bwd_finalize_ex(part.data_ptr(), c, per, gd.data_ptr(), mean_d.data_ptr(), invstd_d.data_ptr(), coef.data_ptr(),
                                         None if null else dgam.data_ptr(), None if null else dbet.data_ptr(), acc, groups, blocks, aff, sp()))
        what = f"(accumulate {acc}, affine_groups {aff}, null {null}, blocks {blocks})"
        cf = coef.cpu().double().view(groups, 3, c)
        for k in range(groups):                                         # a group reading its neighbour's sums or statistics fails here
            R.close(cf[k, 0], A[k], 5e-4, f"A group {k} {what}", per_channel=True)
            R.close(cf[k, 1], B[k], 5e-4, f"B group {k} {what}", per_channel=True)
            R.close(cf[k, 2], C[k], 5e-4, f"C group {k} {what}", per_channel=True)
        if coef0 is None:
            coef0 = coef
        assert same_bits(coef, coef0), f"coefficients depend on {what}"
        if null:
            assert same_bits(dgam, vec(dg0)) and same_bits(dbet, vec(db0))
        else:
            dg_ref, db_ref = R.bwd_dparams(sum_g, sum_gx, dg0, db0, bool(acc), aff)
            R.close(dgam, dg_ref, 5e-4, f"dgamma {what}", per_channel=True)
            R.close(dbet, db_ref, 5e-4, f"dbeta {what}", per_channel=True)

    # ---- apply
    for dk in ds_kinds:
        ds16 = st["ds"] if dk == "same" else 0
        dx = out_like(dyd, st["dx"])
        ds_a = out_like(dyd, ds16) if dk else None
        m = (_mask(st) & 0b10111) | (ds16 << 3)
        check(lib.ctl_bwd_apply_dt(mode, dyd.data_ptr(), actd.data_ptr() if mode == 0 else None, ud.data_ptr(),
                                   scale_d.data_ptr() if mode == 1 else None, shift_d.data_ptr() if mode == 1 else None, SLOPE, coef0.data_ptr(),
                                   M, c, ops.ptr(ds_a), dx.data_ptr(), groups, m, sp()))
        got = dx.cpu().double()
        if amb is not None:
            got = torch.where(amb, dx_ref, got)
        R.close(got, dx_ref, 5e-4, f"dx (ds {dk})", per_channel=True, bf16_out=bool(st["dx"]))
        if dk:
            R.close(ds_a, g_ref, 1e-5, f"ds of the apply pass ({dk})", per_channel=True, bf16_out=bool(ds16))


def test_bn_backward_launchers_refuse_bad_arguments():
    """refused before anything is launched: a channel count the reduction cannot split (c = 12), ds outside mode 0"""
    x = torch.zeros(2, 16, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    part = torch.empty(lib.ctl_red_blocks() * 2 * 16, device=DEV)
    for mode in (0, 1, 2):
        with pytest.raises(CtlError):
            check(lib.ctl_bwd_reduce_dt(mode, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), SLOPE, 32, 12, part.data_ptr(), 1, 0,
                                        None, sp()))
    for mode in (1, 2):
        with pytest.raises(CtlError):
            check(lib.ctl_bwd_reduce_dt(mode, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), SLOPE, 32, 16, part.data_ptr(), 1, 0,
                                        x.data_ptr(), sp()))


# ================================================================================================ b. forms that must agree bit for bit
def _rand_bf16(shape, g, scale=1.0, shift=0.0):
    return R.rb(torch.randn(*shape, generator=g, dtype=F64) * scale + shift)


BIT_SHAPES = [((1, 8, 3, 3), 1), ((3, 8, 5, 7), 1), ((3, 8, 5, 7), 3), ((2, 8, 3, 3), 2), ((2, 64, 6, 6), 2), ((2, 128, 4, 4), 1), ((4, 16, 64, 64), 2),
              ((6, 32, 9, 7), 3), (BIG, 2)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape,groups", BIT_SHAPES)
def test_bwd_apply_16byte_kernel_is_bitwise_the_quad_kernel(mode, shape, groups):
    """all-bf16 tensors take bwd_apply16_kernel; asking for an fp32 dx (and ds) takes bwd_apply_kernel on the same data.  Same arithmetic,
    same rounding points: the fp32 result rounded to bf16 on the host (RNE) must be the 16-byte kernel's output, bit for bit."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(mode * 100 + c + h + groups)
    dy, act, u = (nhwc(_rand_bf16(shape, g, s, o), True) for s, o in ((1.0, 0.1), (1.0, 0.0), (1.5, 0.7)))
    coef = vec(torch.randn(groups, 3, c, generator=g, dtype=F64))        # every group its own coefficients
    scale, shift = vec(torch.rand(groups, c, generator=g, dtype=F64) + 0.5), vec(torch.randn(groups, c, generator=g, dtype=F64) * 0.3)
    M = n * h * w
    with_ds = mode == 0

    def run(dx16, ds16):
        dx, ds = out_like(dy, dx16), (out_like(dy, ds16) if with_ds else None)
        m = 1 | 2 | 4 | (8 if ds16 else 0) | (16 if dx16 else 0)
        check(lib.ctl_bwd_apply_dt(mode, dy.data_ptr(), act.data_ptr() if mode == 0 else None, u.data_ptr(), scale.data_ptr() if mode == 1 else None,
                                   shift.data_ptr() if mode == 1 else None, SLOPE, coef.data_ptr(), M, c, ops.ptr(ds), dx.data_ptr(), groups, m, sp()))
        return dx, ds

    dx16, ds16 = run(True, True)
    dx32, ds32 = run(False, False)
    assert same_bits(dx16, dx32.to(torch.bfloat16)), "dx"
    if with_ds:
        assert same_bits(ds16, ds32.to(torch.bfloat16)), "ds"
        dxq, dsq = run(True, False)                                      # fp32 ds alone sends bf16 tensors to the quad kernel
        assert same_bits(dxq, dx16) and same_bits(dsq, ds32)
        dx_no = out_like(dy, True)                                       # without ds
        check(lib.ctl_bwd_apply_dt(0, dy.data_ptr(), act.data_ptr(), u.data_ptr(), None, None, SLOPE, coef.data_ptr(), M, c, None, dx_no.data_ptr(),
                                   groups, 1 | 2 | 4 | 16, sp()))
        assert same_bits(dx_no, dx16)
    # and the values themselves, against float64 (per group: a group reading its neighbour's coefficients fails)
    cf, dyv, uv = R.f64(coef).view(groups, 3, c), R.f64(dy), R.f64(u)
    gg = R.bwd_g(mode, dyv, act_src=R.f64(act), u=uv, scale=R.f64(scale).view(groups, c), shift=R.f64(shift).view(groups, c), slope=SLOPE, groups=groups)
    ref = R.bwd_apply(gg, uv, cf[:, 0], cf[:, 1], cf[:, 2], groups)
    got = dx32.cpu().double()
    if mode == 1:
        got = torch.where(_sign_ambiguous(uv, R.f64(scale).view(groups, c), R.f64(shift).view(groups, c), groups), ref, got)
    per = n // groups
    for k in range(groups):
        R.close(got[k * per:(k + 1) * per], ref[k * per:(k + 1) * per], 1e-5, f"dx of group {k}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape,groups", BIT_SHAPES)
def test_bwd_reduce_16byte_kernel_against_quad_kernel(mode, shape, groups):
    """the two forms split the pixels differently between threads, so their rows differ; the float64 sum over the rows of each must be the
    reference sum, and the two must agree at the forward-statistics tolerance"""
    n, c, h, w = shape
    M, per = n * h * w, n * h * w // groups
    rows = lib.ctl_bwd_reduce_rows(mode, per, c)
    for attempt in range(4):
        g = torch.Generator().manual_seed(mode * 100 + c + h + groups + 7 + 7919 * attempt)
        dyv, actv, uv = _rand_bf16(shape, g, 1.0, 1.0), _rand_bf16(shape, g), _rand_bf16(shape, g, 1.5, 1.5)
        sc, sh = torch.rand(groups, c, generator=g, dtype=F64) + 0.5, torch.randn(groups, c, generator=g, dtype=F64) * 0.3
        g_ref = R.bwd_g(mode, dyv, act_src=actv, u=uv, scale=q32(sc), shift=q32(sh), slope=SLOPE, groups=groups)
        s1, s2 = R.bwd_sums(g_ref, uv, groups)
        a1, a2 = R.bwd_sums(g_ref.abs(), uv.abs(), groups)
        if _definite(s1, a1, 2e-4, _sum_T(per, c, mode)) and _definite(s2, a2, 2e-4, _sum_T(per, c, mode)):      # (see _definite: the reference only)
            break
    else:
        raise AssertionError("no draw with definite per-channel sums")
    dy16, dy32, act, u = nhwc(dyv, True), nhwc(dyv, False), nhwc(actv, True), nhwc(uv, True)
    scale, shift = vec(sc), vec(sh)
    sums = []
    for dyd, m in ((dy16, 7), (dy32, 6)):                                # fp32 dy: the quad kernel on otherwise bf16 tensors
        part = torch.empty(groups * rows * 2 * c, device=DEV)
        check(lib.ctl_bwd_reduce_dt(mode, dyd.data_ptr(), act.data_ptr() if mode == 0 else None, u.data_ptr(), scale.data_ptr() if mode == 1 else None,
                                    shift.data_ptr() if mode == 1 else None, SLOPE, M, c, part.data_ptr(), groups, m, None, sp()))
        sums.append(part.cpu().double().view(groups, rows, 2, c).sum(1))
        R.close(sums[-1][:, 0], s1, 2e-4, f"sum g (mask {m})", per_channel=True)
        R.close(sums[-1][:, 1], s2, 2e-4, f"sum g*u (mask {m})", per_channel=True)
    R.close(sums[0], sums[1], 2e-4, "16-byte against quad", per_channel=True)


@pytest.mark.parametrize("shape,groups", [((2, 8, 3, 3), 2), ((2, 16, 5, 7), 2), ((4, 4, 3, 3), 2), ((3, 32, 9, 7), 1), ((6, 8, 5, 3), 3), ((2, 128, 4, 4), 1), (BIG, 2)])
def test_bn_act_dt_storage_forms(shape, groups):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c + h + groups)
    mag = 10.0 ** (torch.rand(c, generator=g, dtype=F64) * 2 - 1)
    xv = torch.randn(n, c, h, w, generator=g, dtype=F64) * mag.view(1, -1, 1, 1)
    sc = q32((torch.rand(groups, c, generator=g, dtype=F64) + 0.5) / mag)          # two (three) different coefficient sets
    sh = q32(torch.randn(groups, c, generator=g, dtype=F64) * 0.5)
    scale, shift = vec(sc), vec(sh)
    M = n * h * w
    out = {}
    for x16 in (0, 1):
        xs = R.rb(xv) if x16 else q32(xv)
        xd = nhwc(xs, x16)
        ref = R.bn_act(xs, sc, sh, SLOPE, groups)
        for y16 in (0, 1):
            y = out_like(xd, y16)
            check(lib.ctl_bn_act_dt(xd.data_ptr(), scale.data_ptr(), shift.data_ptr(), SLOPE, y.data_ptr(), M, c, groups, x16 | y16 << 1, sp()))
            R.close(y, ref, 1e-5, f"bn_act x16={x16} y16={y16}", bf16_out=bool(y16))
            per = n // groups
            for k in range(groups):
                R.close(y[k * per:(k + 1) * per], ref[k * per:(k + 1) * per], 1e-5, f"bn_act group {k} x16={x16} y16={y16}", bf16_out=bool(y16))
            out[x16, y16] = y
        if not x16:
            y0 = out_like(xd, 0)
            check(lib.ctl_bn_act(xd.data_ptr(), scale.data_ptr(), shift.data_ptr(), SLOPE, y0.data_ptr(), M, c, groups, sp()))
            assert same_bits(y0, out[0, 0])
    assert same_bits(out[1, 1], out[1, 0].to(torch.bfloat16)), "bf16 -> bf16 against the host rounding of bf16 -> fp32"
    assert same_bits(out[0, 1], out[0, 0].to(torch.bfloat16)), "fp32 -> bf16 against the host rounding of fp32 -> fp32"


# ================================================================================================ c. BatchNorm forward finalize
def _stat_inputs(shape, g):
    """channels of different magnitude whose means keep away from zero (a per-channel relative bound on the mean needs that), parameters
    and running statistics signed so that shift and the running mean are sums of like-signed terms"""
    n, c, h, w = shape
    sig = 10.0 ** (torch.rand(c, generator=g, dtype=F64) * 2 - 1)
    sgn = torch.where(torch.rand(c, generator=g, dtype=F64) < 0.5, -1.0, 1.0).to(F64)
    mu = sig * (torch.rand(c, generator=g, dtype=F64) * 1.5 + 0.5) * sgn
    x = q32(torch.randn(n, c, h, w, generator=g, dtype=F64) * sig.view(1, -1, 1, 1) + mu.view(1, -1, 1, 1))
    gamma = q32(torch.rand(c, generator=g, dtype=F64) + 0.5)
    beta = q32(-(torch.rand(c, generator=g, dtype=F64) + 0.5) * sgn)
    rm = q32(mu * (torch.rand(c, generator=g, dtype=F64) + 0.5))
    rv = q32(sig * sig * (torch.rand(c, generator=g, dtype=F64) + 0.5))
    return x, gamma, beta, rm, rv


def _forward_partials(xd, n, c, h, w, groups):
    M = n * h * w
    rows = lib.ctl_bwd_reduce_rows(0, M // groups, c)
    part = torch.empty(groups * rows * 2 * c, device=DEV)
    ones = torch.ones_like(xd)
    check(lib.ctl_bwd_reduce(0, xd.data_ptr(), ones.data_ptr(), xd.data_ptr(), None, None, SLOPE, M, c, part.data_ptr(), groups, sp()))
    torch.cuda.synchronize()
    return part, rows


@pytest.mark.parametrize("shape,groups", [((6, 16, 9, 7), 1), ((6, 16, 9, 7), 2), ((6, 16, 9, 7), 3), ((3, 128, 4, 4), 3), ((4, 4, 32, 32), 2), ((2, 8, 3, 3), 1)])
def test_bn_finalize_ex_groups_running_update_and_save_uvar(shape, groups):
    n, c, h, w = shape
    x, gamma, beta, rm, rv = _stat_inputs(shape, torch.Generator().manual_seed(c + groups))
    xd, gd, bd = nhwc(x), vec(gamma), vec(beta)
    part, rows = _forward_partials(xd, n, c, h, w, groups)
    count = n * h * w // groups
    ref = R.bn_finalize(x, gamma, beta, EPS, MOM, rm, rv, nbt=5, groups=groups)

    def run(update):
        rmd, rvd, nbt = vec(rm), vec(rv), torch.tensor([5], dtype=torch.int64, device=DEV)
        o = {k: torch.full((groups * c,), float("nan"), device=DEV) for k in ("scale", "shift", "mean", "invstd", "uvar")}
        check(lib.ctl_bn_finalize_ex(part.data_ptr(), rows, c, count, gd.data_ptr(), bd.data_ptr(), EPS, MOM, update, rmd.data_ptr(), rvd.data_ptr(),
                                     nbt.data_ptr(), o["scale"].data_ptr(), o["shift"].data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr(),
                                     o["uvar"].data_ptr(), groups, sp()))
        return o, rmd, rvd, nbt

    o, rmd, rvd, nbt = run(1)
    for k in ("scale", "shift", "mean", "invstd", "uvar"):
        R.close(o[k].view(groups, c), ref[k], 1e-5, k, per_channel=True)
    R.close(rmd, ref["running_mean"], 1e-5, "running_mean after the groups in order", per_channel=True)
    R.close(rvd, ref["running_var"], 1e-5, "running_var after the groups in order", per_channel=True)
    assert int(nbt.item()) == 5 + groups == ref["nbt"]
    if groups > 1:      # the order matters: the update applied in reverse gives something else, and the test would see it
        wrong = R.bn_finalize(x.flip(0), gamma, beta, EPS, MOM, rm, rv, groups=groups)["running_mean"]
        assert R.rel_err(wrong, ref["running_mean"], per_channel=True) > 1e-4
    o0, rm0, rv0, nbt0 = run(0)
    assert same_bits(rm0, vec(rm)) and same_bits(rv0, vec(rv)) and int(nbt0.item()) == 5, "update_running = 0 touched the buffers"
    for k in ("scale", "shift", "mean", "invstd"):
        assert same_bits(o0[k], o[k])
    # ctl_bn_finalize is the same launch without save_uvar
    rmd2, rvd2, nbt2 = vec(rm), vec(rv), torch.tensor([5], dtype=torch.int64, device=DEV)
    sc2, sh2, mean2, is2 = ops.bn_finalize(part, c, count, gd, bd, EPS, MOM, rmd2, rvd2, nbt2, groups)
    assert same_bits(sc2, o["scale"]) and same_bits(sh2, o["shift"]) and same_bits(mean2, o["mean"]) and same_bits(is2, o["invstd"]) and same_bits(rmd2, rmd)


@pytest.mark.parametrize("c,groups", [(4, 1), (16, 2), (130, 3)])
def test_bn_eval_coeffs(c, groups):
    g = torch.Generator().manual_seed(c)
    _, gamma, beta, rm, rv = _stat_inputs((1, c, 1, 1), g)
    gd, bd, rmd, rvd = vec(gamma), vec(beta), vec(rm), vec(rv)
    scale, shift = torch.full((groups * c,), float("nan"), device=DEV), torch.full((groups * c,), float("nan"), device=DEV)
    check(lib.ctl_bn_eval_coeffs(c, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), EPS, scale.data_ptr(), shift.data_ptr(), groups, sp()))
    sc, sh = R.bn_eval_coeffs(gamma, beta, rm, rv, EPS, groups)
    R.close(scale.view(groups, c), sc, 1e-6, "eval scale", per_channel=True)
    R.close(shift.view(groups, c), sh, 1e-6, "eval shift", per_channel=True)
    for k in range(1, groups):
        assert same_bits(scale.view(groups, c)[k], scale.view(groups, c)[0]) and same_bits(shift.view(groups, c)[k], shift.view(groups, c)[0])


def test_bn_replay_running_from_a_hand_built_table():
    """two records {mean byte offset, uvar byte offset, running_mean float offset, running_var float offset, nbt index, c}.  First with data on
    which every product and sum is exact (bit-equal), then with momentum 0.1 and random data within 1 ulp of (1-m)*rm + m*mean: a fused
    evaluation rounds twice (<= 1 ulp); an unfused one rounds both products and the sum, 1/2 ulp(sum) + 1/2 ulp(first product) + 1/2
    ulp(second product), where the operands are like-signed, the first product is under the sum and the second under a quarter of it:
    1/2 + 1/2 + 1/8 ulp in the worst alignment of all three roundings, which these 292 values do not meet."""
    g = torch.Generator().manual_seed(11)
    c0, c1 = 16, 130
    for exact in (True, False):
        if exact:      # momentum 1/4 and values on a 2^-8 grid: every product and sum is exact in fp32, fused or not
            mom = 0.25
            draw = lambda k, pos=False: torch.randint(1 if pos else -1024, 1024, (k,), generator=g).to(F64) / 256
        else:
            mom = MOM
            draw = lambda k, pos=False: q32(torch.rand(k, generator=g, dtype=F64) + 0.5) * (1 if pos else -1)      # like-signed terms
        mean0, uvar0, mean1, uvar1 = draw(c0), draw(c0, True), draw(c1), draw(c1, True)
        rm0, rv0, rm1, rv1 = draw(c0), draw(c0, True), draw(c1), draw(c1, True)
        pad = torch.zeros(3, dtype=F64)
        act = vec(torch.cat([pad, mean1, uvar0, pad, mean0, uvar1]))
        o_mean1, o_uvar0, o_mean0, o_uvar1 = 3, 3 + c1, 6 + c1 + c0, 6 + c1 + 2 * c0
        buf_cpu = torch.cat([rv1, pad, rm0, rm1, rv0])
        buffers = vec(buf_cpu)
        o_rv1, o_rm0, o_rm1, o_rv0 = 0, c1 + 3, c1 + 3 + c0, 2 * c1 + 3 + c0
        nbt = torch.tensor([7, 100, 41], dtype=torch.int64, device=DEV)
        table = torch.tensor([[4 * o_mean0, 4 * o_uvar0, o_rm0, o_rv0, 2, c0], [4 * o_mean1, 4 * o_uvar1, o_rm1, o_rv1, 0, c1]], dtype=torch.int64, device=DEV)
        check(lib.ctl_bn_replay_running(act.data_ptr(), buffers.data_ptr(), nbt.data_ptr(), table.data_ptr(), 2, mom, sp()))
        assert nbt.tolist() == [8, 100, 42]
        got = buffers.cpu()
        m32 = float(np.float32(mom))
        keep = float(np.float32(1.0) - np.float32(mom))                 # (1 - momentum) is formed in fp32
        for name, off, old, new in (("rm0", o_rm0, rm0, mean0), ("rv0", o_rv0, rv0, uvar0), ("rm1", o_rm1, rm1, mean1), ("rv1", o_rv1, rv1, uvar1)):
            ref = keep * old + m32 * new
            val = got[off:off + len(old)].double()
            if exact:
                assert torch.equal(val, ref), name
            else:
                ulp = torch.from_numpy(np.spacing(ref.abs().numpy().astype(np.float32))).double()
                assert bool(((val - ref).abs() <= ulp).all()), (name, float(((val - ref).abs() / ulp).max()))
        assert torch.equal(got[c1:c1 + 3].double(), pad), "wrote outside the records"


def _reduce_T(per_group_pixels, c):
    """fp32 additions behind one entry of a partial row: the trips of one thread plus the EB / (c/4) threads of the block that hold the channel"""
    cq = c // 4
    rows = lib.ctl_bwd_reduce_rows(0, per_group_pixels, c)
    quads = per_group_pixels * cq
    trips = -(-quads // (rows * EB))
    return trips + EB // cq


@pytest.mark.parametrize("r", [0, 8, 32])
@pytest.mark.parametrize("shape", [(2, 16, 32, 32), (2, 128, 4, 4), BIG])
def test_forward_statistics_conditioning(r, shape):
    """mean / std = r.  The partial rows are fp32 sums of x and of x*x (positive terms); everything after them is float64.  With T fp32
    additions behind one row entry the sums carry at most T * 2^-24 of sum|x| and of sum x^2, hence
        |d invstd| / invstd <= 1/2 * T * 2^-24 * (1 + r^2) + 2^-23        |d mean| <= T * 2^-24 * E|x| + 2^-24 * |mean|
    (the last terms: the fp32 stores).  The bound is derived, not measured; the figures are printed for DESIGN.md."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(r + c)
    x32 = torch.randn(n, c, h, w, generator=g) + float(r)                # drawn in fp32; the reference sees the same values
    x = x32.double()
    xd = nhwc(x)
    part, rows = _forward_partials(xd, n, c, h, w, 1)
    M = n * h * w
    ones = vec(torch.ones(c, dtype=F64))
    zeros = vec(torch.zeros(c, dtype=F64))
    scale, shift, mean, invstd = (torch.empty(c, device=DEV) for _ in range(4))
    check(lib.ctl_bn_finalize_ex(part.data_ptr(), rows, c, M, ones.data_ptr(), zeros.data_ptr(), EPS, MOM, 0, None, None, None, scale.data_ptr(),
                                 shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), None, 1, sp()))
    ref = R.bn_finalize(x, ones, zeros, EPS, MOM, groups=1, update_running=False)
    T = _reduce_T(M, c)
    rr2 = ref["mean"][0] ** 2 / ref["var"][0]
    e_abs = x.abs().mean((0, 2, 3))
    d_is = ((invstd.cpu().double() - ref["invstd"][0]).abs() / ref["invstd"][0])
    d_mu = (mean.cpu().double() - ref["mean"][0]).abs()
    b_is = 0.5 * T * U24 * (1 + rr2) + 2.0 ** -23
    b_mu = T * U24 * e_abs + U24 * ref["mean"][0].abs()
    print(f"conditioning r={r} shape={shape} T={T}: max |d invstd|/invstd {float(d_is.max()):.3e} (bound {float(b_is.min()):.3e}), "
          f"max |d mean| {float(d_mu.max()):.3e} (bound {float(b_mu.min()):.3e})")
    assert bool((d_is <= b_is).all()), (float(d_is.max()), float(b_is.min()))
    assert bool((d_mu <= b_mu).all()), (float(d_mu.max()), float(b_mu.min()))


# ================================================================================================ d. additions only: exact
def _pool_ref32(x):
    """(a0 + a1) + (a2 + a3) in fp32: a0, a1 the upper pixel pair, a2, a3 the lower"""
    x = x.float()
    return (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])


@pytest.mark.parametrize("n,c,h,w", [(2, 4, 3, 5), (1, 8, 1, 1), (3, 16, 7, 9), (2, 128, 2, 3), (4, 16, 192, 192)])
def test_sumpool2_is_exact(n, c, h, w):
    """(h, w) is the pooled size.  The last case has more quads than one grid pass covers."""
    if h == 192:
        assert n * h * w * (c // 4) > MAX_STREAM_BLOCKS * EB
    g = torch.Generator().manual_seed(c + h)
    up = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    prev = torch.randn(n, c, h, w, generator=g)
    upd = nhwc(up)
    dx = nhwc(prev)
    check(lib.ctl_sumpool2(upd.data_ptr(), dx.data_ptr(), n, h, w, c, 0, sp()))
    assert torch.equal(dx.cpu(), _pool_ref32(up))
    dx = nhwc(prev)
    check(lib.ctl_sumpool2(upd.data_ptr(), dx.data_ptr(), n, h, w, c, 1, sp()))
    assert torch.equal(dx.cpu(), _pool_ref32(up) + prev)
    R.close(dx, R.sumpool2(up) + prev.double(), 1e-6, "sum-pool against float64")
    # bf16 input: the fp32 sum of the bf16 values, rounded once where the output is bf16
    up16 = up.to(torch.bfloat16)
    up16d = nhwc(up16, True)
    s32 = _pool_ref32(up16)
    for out16 in (1, 0):
        o = out_like(dx, out16)
        check(lib.ctl_sumpool2_dt(up16d.data_ptr(), o.data_ptr(), n, h, w, c, 0, 1 | out16 << 1, sp()))
        assert same_bits(o.cpu(), s32.to(torch.bfloat16) if out16 else s32), f"ctl_sumpool2_dt bf16 in, out16={out16}"
        p = prev.to(torch.bfloat16) if out16 else prev
        o = nhwc(p, out16)
        check(lib.ctl_sumpool2_dt(up16d.data_ptr(), o.data_ptr(), n, h, w, c, 1, 1 | out16 << 1, sp()))
        acc = s32 + p.float()
        assert same_bits(o.cpu(), acc.to(torch.bfloat16) if out16 else acc), f"ctl_sumpool2_dt accumulate, out16={out16}"


@pytest.mark.parametrize("n,c,h,w", [(1, 8, 3, 3), (3, 4, 5, 7), (2, 128, 4, 4), (4, 32, 48, 40), (16, 16, 128, 128)])
def test_chan_sum_finalize_with_and_without_accumulate(n, c, h, w):
    g = torch.Generator().manual_seed(c + h)
    mag = 10.0 ** (torch.rand(c, generator=g, dtype=F64) * 3 - 2)
    dy = q32((torch.randn(n, c, h, w, generator=g, dtype=F64) + 0.5) * mag.view(1, -1, 1, 1))
    prev = q32(torch.rand(c, generator=g, dtype=F64) * mag)
    dyd = nhwc(dy)
    ref = R.bwd_sums(R.bwd_g(2, dy))[0][0]
    rows = lib.ctl_bwd_reduce_rows(2, n * h * w, c)
    assert rows == lib.ctl_red_blocks()
    outs = []
    for rep in range(2):
        part = torch.empty(rows * 2 * c, device=DEV)
        check(lib.ctl_bwd_reduce_dt(2, dyd.data_ptr(), None, None, None, None, 0.0, n * h * w, c, part.data_ptr(), 1, 0, None, sp()))
        o0, o1 = torch.full((c,), float("nan"), device=DEV), vec(prev)
        check(lib.ctl_chan_sum_finalize(part.data_ptr(), c, o0.data_ptr(), 0, sp()))
        check(lib.ctl_chan_sum_finalize(part.data_ptr(), c, o1.data_ptr(), 1, sp()))
        R.close(o0, ref, 2e-4, "channel sums", per_channel=True)
        R.close(o1, ref + prev, 2e-4, "channel sums on top of the previous value", per_channel=True)
        assert torch.equal(o1.cpu(), prev.float() + o0.cpu())
        outs.append((o0, o1))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "not reproducible"
    # bf16 storage of dy: same sums of the rounded values
    dy16 = R.rb(dy)
    d16 = nhwc(dy16, True)
    part = torch.empty(rows * 2 * c, device=DEV)
    check(lib.ctl_bwd_reduce_dt(2, d16.data_ptr(), None, None, None, None, 0.0, n * h * w, c, part.data_ptr(), 1, 1, None, sp()))
    o = torch.empty(c, device=DEV)
    check(lib.ctl_chan_sum_finalize(part.data_ptr(), c, o.data_ptr(), 0, sp()))
    R.close(o, dy16.sum((0, 2, 3)), 2e-4, "channel sums of a bf16 tensor", per_channel=True)


@pytest.mark.parametrize("count", [1, 255, 257, MAX_STREAM_BLOCKS * EB * 2 + 3])
@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_accumulate_is_the_ordered_fp32_sum(k, count):
    g = torch.Generator().manual_seed(k + count % 1000)
    dst = torch.randn(count, generator=g)
    srcs = [torch.randn(count, generator=g) * 10.0 ** (j % 3 - 1) for j in range(k)]
    dd, sd = dst.to(DEV), [s.to(DEV) for s in srcs]
    arr = (ctypes.c_void_p * k)(*[s.data_ptr() for s in sd])
    check(lib.ctl_accumulate(dd.data_ptr(), arr, k, count, sp()))
    ref = dst.clone()
    for s in srcs:
        ref = ref + s                                                    # ((dst + s0) + s1) + ... in fp32
    assert torch.equal(dd.cpu(), ref)
    R.close(dd, R.accumulate(dst, srcs), 1e-6, "accumulate against float64")


def test_accumulate_refuses_k_out_of_range():
    d = torch.zeros(16, device=DEV)
    arr = (ctypes.c_void_p * 9)(*[d.data_ptr()] * 9)
    for k in (0, 9):
        with pytest.raises(CtlError):
            check(lib.ctl_accumulate(d.data_ptr(), arr, k, 16, sp()))
    assert float(d.abs().max()) == 0.0


# ================================================================================================ e. STN builders and losses
PIXELS = [1, 255, 257, 3 * 24 * 20, 16 * 256 * 256]
MAXC = 16


def _nchw(rows):
    """[pixels, c] rows (the kernels' layout) -> [1, c, pixels, 1] for the reference"""
    return rows.t().reshape(1, rows.shape[1], rows.shape[0], 1)


def _rows(t):
    return t.reshape(t.shape[1], t.shape[2]).t()


def _logits(pixels, c, scale, g):
    x = torch.randn(pixels, c, generator=g) * scale
    ties = {}
    if pixels >= 255 and c > 1:
        x[0:10] = (torch.randn(10, 1, generator=g) * scale).expand(10, c)            # all-equal rows
        for i in range(10, 40):                                                       # an exact two-way tie for the maximum
            a, b = sorted(torch.randperm(c, generator=g)[:2].tolist())
            top = float(x[i].abs().max()) + 1.0
            x[i, a] = top
            x[i, b] = top
            ties[i] = a
    return x, ties


@pytest.mark.parametrize("scale", [3.0, 200.0])
@pytest.mark.parametrize("pixels", PIXELS)
@pytest.mark.parametrize("c", [1, 2, 3, 4, 7, 16])
def test_softmax_onehot_argmax_cross_entropy(c, pixels, scale):
    g = torch.Generator().manual_seed(c * 7 + pixels % 1000 + int(scale))
    x, ties = _logits(pixels, c, scale, g)
    lab = torch.randint(0, c, (pixels,), generator=g)
    xd, labd = x.to(DEV), lab.to(DEV)
    xr = _nchw(x.double())
    # softmax, T = 2 (at scale 200 expf overflows unless the row maximum is taken off first)
    p = torch.full_like(xd, float("nan"))
    check(lib.ctl_softmax_t_fwd(xd.data_ptr(), 0.5, p.data_ptr(), pixels, c, sp()))
    pc = p.cpu()
    assert bool(torch.isfinite(pc).all())
    assert float((pc.double().sum(1) - 1).abs().max()) <= 4 * U24 * c
    R.close(_nchw(pc.double()), R.softmax_t_fwd(xr, 2.0), 1e-6, "softmax T=2")
    if ties:
        assert bool((pc[0:10] == pc[0:10, :1]).all()) and float((pc[0:10].double() - 1.0 / c).abs().max()) <= 2 * U24 / c, "all-equal rows: uniform"
        for i, a in ties.items():
            assert float(pc[i].max()) == float(pc[i, a])
    dp = torch.randn(pixels, c, generator=g)
    dpd = dp.to(DEV)
    dx = torch.full_like(xd, float("nan"))
    check(lib.ctl_softmax_t_bwd(p.data_ptr(), dpd.data_ptr(), 0.5, dx.data_ptr(), pixels, c, sp()))
    assert bool(torch.isfinite(dx).all())
    R.close(_nchw(dx.cpu().double()), R.softmax_t_bwd(_nchw(pc.double()), _nchw(dp.double()), 2.0), 1e-5, "softmax backward")
    # one-hot and argmax: exact
    y = torch.full_like(xd, float("nan"))
    check(lib.ctl_onehot(labd.data_ptr(), y.data_ptr(), pixels, c, sp()))
    assert torch.equal(_nchw(y.cpu().double()), R.onehot(lab.view(1, pixels, 1), c))
    am = torch.full((pixels,), 255, dtype=torch.uint8, device=DEV)
    check(lib.ctl_argmax_c(xd.data_ptr(), am.data_ptr(), pixels, c, sp()))
    assert np.array_equal(am.cpu().numpy(), np.argmax(x.numpy(), axis=1).astype(np.uint8)), "argmax is the first maximum"
    assert torch.equal(am.cpu(), R.argmax_first(xr).view(-1))
    for i, a in ties.items():
        assert int(am[i]) == a
    # cross-entropy: float64 partials, so the size costs nothing
    part = torch.empty(lib.ctl_red_blocks(), dtype=F64, device=DEV)
    loss = torch.full((), float("nan"), device=DEV)
    check(lib.ctl_ce2d_fwd(xd.data_ptr(), labd.data_ptr(), pixels, c, part.data_ptr(), loss.data_ptr(), sp()))
    ref = R.ce_mean(xr, lab.view(1, pixels, 1))
    assert np.isfinite(float(loss)) and abs(float(loss) - ref) <= 2e-6 * max(1.0, abs(ref)), (float(loss), ref)
    gout = torch.tensor(0.7, device=DEV)
    dl = torch.full_like(xd, float("nan"))
    check(lib.ctl_ce2d_bwd(xd.data_ptr(), labd.data_ptr(), gout.data_ptr(), pixels, c, dl.data_ptr(), sp()))
    assert bool(torch.isfinite(dl).all())
    R.close(_nchw(dl.cpu().double()), R.ce_grad(xr, lab.view(1, pixels, 1), float(np.float32(0.7))), 1e-5, "cross-entropy backward")


@pytest.mark.parametrize("pixels", [1, 255, 257, 16 * 256 * 256])
def test_c4_runtime_count_kernel_is_bitwise_the_16byte_kernel(pixels):
    """rows of 4 channels take the 16-byte-row kernels only when every pointer is 16-byte aligned.  Views at storage offset 1 of a larger
    buffer (4 bytes off) take the runtime-count kernels: same arithmetic in the same order, so the same bits."""
    g = torch.Generator().manual_seed(pixels % 1000)
    x = torch.randn(pixels, 4, generator=g) * 3
    dp = torch.randn(pixels, 4, generator=g)
    lab = torch.randint(0, 4, (pixels,), generator=g).to(DEV)
    gout = torch.tensor(0.7, device=DEV)

    def off1(t=None):
        buf = torch.zeros(pixels * 4 + 8, device=DEV)                    # keeps the view's storage alive
        v = buf[1:1 + pixels * 4].view(pixels, 4)
        if t is not None:
            v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    def run(al):
        mk = (lambda t=None: (torch.zeros(pixels, 4, device=DEV) if t is None else t.to(DEV).contiguous())) if al else off1
        xd, dpd, p, dx, dl = mk(x), mk(dp), mk(), mk(), mk()
        if al:
            assert all(t.data_ptr() % 16 == 0 for t in (xd, dpd, p, dx, dl))
        check(lib.ctl_softmax_t_fwd(xd.data_ptr(), 0.5, p.data_ptr(), pixels, 4, sp()))
        check(lib.ctl_softmax_t_bwd(p.data_ptr(), dpd.data_ptr(), 0.5, dx.data_ptr(), pixels, 4, sp()))
        part = torch.empty(lib.ctl_red_blocks(), dtype=F64, device=DEV)
        loss = torch.empty((), device=DEV)
        check(lib.ctl_ce2d_fwd(xd.data_ptr(), lab.data_ptr(), pixels, 4, part.data_ptr(), loss.data_ptr(), sp()))
        check(lib.ctl_ce2d_bwd(xd.data_ptr(), lab.data_ptr(), gout.data_ptr(), pixels, 4, dl.data_ptr(), sp()))
        torch.cuda.synchronize()
        return p.clone(), dx.clone(), loss.clone(), dl.clone(), part.clone()

    for name, a, b in zip(("softmax", "softmax backward", "cross-entropy", "cross-entropy backward", "cross-entropy partials"), run(True), run(False)):
        assert torch.equal(a, b), name


def test_row_kernels_refuse_more_than_maxc_channels():
    """c = 17 > MAXC: refused by the argument check of every launcher that keeps a pixel's row in registers; nothing is launched"""
    c, pixels = MAXC + 1, 4
    x = torch.zeros(pixels, c, device=DEV)
    lab = torch.zeros(pixels, dtype=torch.int64, device=DEV)
    part = torch.zeros(lib.ctl_red_blocks(), dtype=F64, device=DEV)
    one = torch.ones((), device=DEV)
    out = torch.full((pixels, c), 5.0, device=DEV)
    with pytest.raises(CtlError):
        check(lib.ctl_softmax_t_fwd(x.data_ptr(), 0.5, out.data_ptr(), pixels, c, sp()))
    with pytest.raises(CtlError):
        check(lib.ctl_softmax_t_bwd(x.data_ptr(), x.data_ptr(), 0.5, out.data_ptr(), pixels, c, sp()))
    with pytest.raises(CtlError):
        check(lib.ctl_ce2d_fwd(x.data_ptr(), lab.data_ptr(), pixels, c, part.data_ptr(), one.data_ptr(), sp()))
    with pytest.raises(CtlError):
        check(lib.ctl_ce2d_bwd(x.data_ptr(), lab.data_ptr(), one.data_ptr(), pixels, c, out.data_ptr(), sp()))
    assert float((out - 5.0).abs().max()) == 0.0 and float(one) == 1.0


@pytest.mark.parametrize("scale", [0.5, 1.0])
@pytest.mark.parametrize("count", [1, 257, 16 * 256 * 256])
def test_mse_forward_and_backward(count, scale):
    """per element (a - b) and its square are one fp32 rounding each, the sum is float64, the store fp32: |d loss| <= 4 * 2^-24 * loss"""
    g = torch.Generator().manual_seed(count % 1000)
    a, b = torch.rand(count, generator=g), torch.rand(count, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    part = torch.empty(lib.ctl_red_blocks(), dtype=F64, device=DEV)
    loss = torch.full((), float("nan"), device=DEV)
    check(lib.ctl_mse_fwd(ad.data_ptr(), bd.data_ptr(), count, scale, part.data_ptr(), loss.data_ptr(), sp()))
    ref = R.mse(a, b, scale)
    assert abs(float(loss) - ref) <= 4 * U24 * ref + 1e-45, (float(loss), ref)
    gout = torch.tensor(0.7, device=DEV)
    da = torch.full_like(ad, float("nan"))
    check(lib.ctl_mse_bwd(ad.data_ptr(), bd.data_ptr(), gout.data_ptr(), count, scale, da.data_ptr(), sp()))
    R.close(da, R.mse_grad(a, b, float(np.float32(0.7)), scale), 1e-5, "mse backward")
    # a == b: exactly zero
    check(lib.ctl_mse_fwd(ad.data_ptr(), ad.data_ptr(), count, scale, part.data_ptr(), loss.data_ptr(), sp()))
    check(lib.ctl_mse_bwd(ad.data_ptr(), ad.data_ptr(), gout.data_ptr(), count, scale, da.data_ptr(), sp()))
    assert float(loss) == 0.0 and float(da.abs().max()) == 0.0


@pytest.mark.parametrize("count", [1, 257, MAX_STREAM_BLOCKS * EB + 77])
def test_sigmoid_backward_with_saturated_outputs(count):
    g = torch.Generator().manual_seed(count % 1000)
    y = torch.sigmoid(torch.randn(count, generator=g) * 4)
    y[0] = 0.0
    y[-1] = 1.0 if count > 1 else 0.0
    y[count // 2::1001] = 1.0
    y[count // 3::1003] = 0.0
    dy = torch.randn(count, generator=g)
    yd, dyd = y.to(DEV), dy.to(DEV)
    dx = torch.full_like(yd, float("nan"))
    check(lib.ctl_sigmoid_bwd(dyd.data_ptr(), yd.data_ptr(), dx.data_ptr(), count, sp()))
    R.close(dx, R.sigmoid_bwd(dy, y), 1e-6, "sigmoid backward")
    sat = (y == 0) | (y == 1)
    assert int(sat.sum()) >= 1 and float(dx.cpu()[sat].abs().max()) == 0.0


# ================================================================================================ f. Adam
LR, B1, B2, AEPS = 1e-4, 0.9, 0.999, 1e-8
B1F, B2F, LRF, EPSF = (float(np.float32(v)) for v in (B1, B2, LR, AEPS))           # what the kernel receives


def _adam_grads(pattern, count, g):
    if pattern == "zero":
        return torch.zeros(count)
    if pattern == "tiny":
        return torch.full((count,), 1e-20)
    if pattern == "huge":
        return torch.full((count,), 1e4) * torch.where(torch.rand(count, generator=g) < 0.5, -1.0, 1.0)
    pick = torch.randint(0, 4, (count,), generator=g)
    rnd = torch.randn(count, generator=g) * 0.1
    return torch.where(pick == 0, torch.zeros(count), torch.where(pick == 1, torch.full((count,), 1e-20), torch.where(pick == 2, torch.full((count,), 1e4), rnd)))


@pytest.mark.parametrize("count", [1, 255, 257, 10007, MAX_STREAM_BLOCKS * EB + 5])
@pytest.mark.parametrize("step", [1, 2, 3, 1000, 100000])
def test_adam_host_and_device_step_count(step, count):
    """one step at a time: m and v come from the float64 recursion at step - 1 (its closed form for a constant earlier gradient), so late
    steps, where both bias corrections have run to 1, are tested on their own.  m and v are held to 4 * 2^-24 relative.  Only where the
    reference is under the smallest normal fp32 number (v of the 1e-20 gradient, about 1e-43) may the result be flushed or held with
    subnormal spacing: there, and only there, the bound is 2^-126 absolute."""
    g = torch.Generator().manual_seed(step % 1000 + count % 1000)
    p0 = torch.randn(count, generator=g)
    for pattern in ("zero", "tiny", "huge", "mix"):
        gr = _adam_grads(pattern, count, g)
        gprev = gr * (torch.rand(count, generator=g) + 0.5)              # like-signed: m is then a sum without cancellation
        for gs in (1.0, 0.5, 0.125):
            gp = gprev.double() * gs
            m0 = ((1 - B1F ** (step - 1)) * gp).float()
            v0 = ((1 - B2F ** (step - 1)) * gp * gp).float()
            pr, mr, vr = R.adam(p0, gr, m0, v0, LRF, B1F, B2F, EPSF, step, gs)
            grd = gr.to(DEV)
            res = []
            for form in ("host", "host", "dev"):
                pd, md, vd = p0.to(DEV), m0.to(DEV), v0.to(DEV)
                if form == "host":
                    check(lib.ctl_adam(pd.data_ptr(), grd.data_ptr(), md.data_ptr(), vd.data_ptr(), count, LR, B1, B2, AEPS, step, gs, sp()))
                else:      # {seed, pass, step}: ops.step_tick advances the pass counter and the step count by one
                    state = torch.tensor([123, 7, step - 1], dtype=torch.int64, device=DEV)
                    ops.step_tick(state)
                    assert state.tolist() == [123, 8, step]
                    check(lib.ctl_adam_dev(pd.data_ptr(), grd.data_ptr(), md.data_ptr(), vd.data_ptr(), count, LR, B1, B2, AEPS, state.data_ptr(), gs, sp()))
                    assert state.tolist() == [123, 8, step]
                res.append((pd, md, vd))
            what = f"{pattern} gradient, grad_scale {gs}"
            for k in range(3):
                assert same_bits(res[0][k], res[1][k]), f"two launches differ ({what})"
                assert same_bits(res[0][k], res[2][k]), f"ctl_adam_dev differs from ctl_adam at the same step ({what})"
            pd, md, vd = (t.cpu().double() for t in res[0])
            assert bool(((pd - pr).abs() <= 2e-7 * pr.abs().clamp_min(1.0)).all()), (what, float((pd - pr).abs().max()))
            for name, got, ref in (("m", md, mr), ("v", vd, vr)):
                tol = torch.where(ref.abs() < 2.0 ** -126, torch.full_like(ref, 2.0 ** -126), 4 * U24 * ref.abs())
                assert bool(((got - ref).abs() <= tol).all()), (what, name, float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max()))
            if pattern == "zero":
                assert same_bits(res[0][0], p0.to(DEV)) and float(md.abs().max()) == 0.0 and float(vd.abs().max()) == 0.0, "zero gradient moved p"
            if pattern == "huge" and gs != 1.0:      # the scaled gradient, not the raw one, feeds the moments
                assert float((md - R.adam(p0, gr, m0, v0, LRF, B1F, B2F, EPSF, step, 1.0)[1]).abs().max()) > 1.0
