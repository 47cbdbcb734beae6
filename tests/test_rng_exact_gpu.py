"""The kernels driven by the counter-hash RNG (ctl_uniform, ctl_uniform_dev, ctl_step_tick, ctl_dropout2d / _ex / _dt in
csrc/ctl_mask.hip, ctl_noise_clamp in csrc/ctl_io.hip) through the C ABI with full 64-bit seeds, against the integer restatement in
oracle/ref_rng.py and the dropout / clamp arithmetic of oracle/ref_mask.py and ref_io.py.  The generator is exact integer arithmetic,
so every draw is compared bit for bit; only the device Gaussian of ctl_noise_clamp goes through logf / sqrtf / cosf and is held to a
derived bound (test_noise_clamp_device_noise_within_the_derived_bound)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check, CtlError  # noqa: E402
from oracle import ref_io, ref_mask, ref_rng  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GRID_CAP_ITEMS = 2048 * 256          # one grid pass of the streaming kernels; above it the loop strides
SEEDS = [0, 1, 2 ** 63, 2 ** 64 - 1]


def sp():
    return ops.stream_ptr()


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def as_i64(v):
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


# ================================================================================================ uniform
@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_is_the_top_24_bits_of_splitmix64(seed):
    for count in (1, 255, 256, 257, GRID_CAP_ITEMS + 3):
        out = torch.full((count + 8,), NAN, device=DEV)
        check(lib.ctl_uniform(ptr(out), count, seed, sp()), "ctl_uniform")
        got = out.cpu().numpy()
        ref = ref_rng.hash_uniform(seed, np.arange(count, dtype=np.uint64))
        assert np.array_equal(bits(got[:count]), bits(ref)), (seed, count)
        assert (got[:count] >= 0).all() and (got[:count] < 1).all() and np.isnan(got[count:]).all()


def test_uniform_dev_follows_the_ticked_state():
    """state = [seed, step, adam_step]: ctl_step_tick adds one to [1] and [2] and leaves [0]; ctl_uniform_dev draws with
    state_seed(seed, step, salt)"""
    count = GRID_CAP_ITEMS + 3
    idx = np.arange(count, dtype=np.uint64)
    for seed, step, adam in ((0, 0, 0), (2 ** 63, 41, 7), (2 ** 64 - 1, 2 ** 33, 2 ** 40)):
        state = torch.tensor([as_i64(seed), step, adam], dtype=torch.int64, device=DEV)
        ticks = 0
        for target in (0, 1, 3):
            while ticks < target:
                check(lib.ctl_step_tick(ptr(state), sp()), "ctl_step_tick")
                ticks += 1
            assert state.cpu().tolist() == [as_i64(seed), step + ticks, adam + ticks]
            for salt in (0, 1, 2 ** 32 + 5):
                n = count if (salt == 1 and target == 1) else 257
                out = torch.full((n,), NAN, device=DEV)
                check(lib.ctl_uniform_dev(ptr(out), n, salt, ptr(state), sp()), "ctl_uniform_dev")
                ref = ref_rng.hash_uniform(ref_rng.state_seed(seed, step + ticks, salt), idx[:n])
                assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), (seed, ticks, salt)
            assert state.cpu().tolist() == [as_i64(seed), step + ticks, adam + ticks]          # a draw does not advance the state
    with pytest.raises(CtlError):
        check(lib.ctl_uniform_dev(ptr(out), 4, 0, None, sp()))
    with pytest.raises(CtlError):
        check(lib.ctl_uniform(ptr(out), 0, 0, sp()))


# ================================================================================================ dropout2d
DROP_SHAPES = [(1, 4, 1), (3, 8, 9), (4, 128, 64), (5, 256, 35), (600, 4, 4)]          # (n, c, hw)
PS = [0.0, 0.1, 0.5, 0.9, 0.999]


def _z(n, c, hw, rng, bf16=False):
    z = rng.standard_normal((n, hw, c)).astype(np.float32)
    flat = z.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return ref_mask.from_bf16_bits(ref_mask.to_bf16_bits(z)) if bf16 else z


def _keep_ref(seed, n, c, p):
    u = ref_rng.hash_uniform(seed, np.arange(n * c, dtype=np.uint64)).reshape(n, c)
    return (u >= np.float32(p)).astype(np.float32)


@pytest.mark.parametrize("n,c,hw", DROP_SHAPES)
def test_dropout2d_draws_and_products_are_exact(n, c, hw):
    rng = np.random.default_rng(n * 1000 + c + hw)
    z = _z(n, c, hw, rng)
    z_d = dev(z)
    out, keep_out, full = (torch.empty(n, hw, c, device=DEV), torch.empty(n, c, device=DEV), torch.empty(n, hw, c, device=DEV))

    def fresh():
        for t in (out, keep_out, full):
            t.fill_(NAN)

    for p in PS:
        for seed in SEEDS + [0x0123456789ABCDEF]:
            keep = _keep_ref(seed, n, c, p)
            ref, ref_full = ref_mask.dropout2d(z, keep, p)
            if p == 0.0:
                assert (keep == 1).all() and (ref_full == 1).all()
            fresh()
            check(lib.ctl_dropout2d(ptr(z_d), None, seed, p, ptr(out), ptr(keep_out), n, hw, c, sp()), "ctl_dropout2d")
            assert np.array_equal(bits(keep_out.cpu().numpy()), bits(keep)), (p, seed, "keep")
            assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), (p, seed, "out")
            fresh()
            check(lib.ctl_dropout2d_ex(ptr(z_d), None, seed, None, p, ptr(out), ptr(keep_out), ptr(full), n, hw, c, sp()), "ctl_dropout2d_ex")
            assert np.array_equal(bits(keep_out.cpu().numpy()), bits(keep)) and np.array_equal(bits(out.cpu().numpy()), bits(ref)), (p, seed, "ex")
            assert np.array_equal(bits(full.cpu().numpy()), bits(ref_full)), (p, seed, "mask_full")
        # the state + salt form is the seed form with the reference's state_seed
        seed0, step, salt = 2 ** 64 - 3, 12345, 2 ** 32 + 5
        state = torch.tensor([as_i64(seed0), step, 0], dtype=torch.int64, device=DEV)
        keep = _keep_ref(ref_rng.state_seed(seed0, step, salt), n, c, p)
        ref, ref_full = ref_mask.dropout2d(z, keep, p)
        fresh()
        check(lib.ctl_dropout2d_ex(ptr(z_d), None, salt, ptr(state), p, ptr(out), ptr(keep_out), ptr(full), n, hw, c, sp()), "ctl_dropout2d_ex")
        assert np.array_equal(bits(keep_out.cpu().numpy()), bits(keep)) and np.array_equal(bits(out.cpu().numpy()), bits(ref)), (p, "state")
        assert np.array_equal(bits(full.cpu().numpy()), bits(ref_full))
        # an injected keep is used as it is and echoed
        keep = (rng.random((n, c)) < 0.6).astype(np.float32)
        ref, ref_full = ref_mask.dropout2d(z, keep, p)
        fresh()
        check(lib.ctl_dropout2d_ex(ptr(z_d), ptr(dev(keep)), 99, None, p, ptr(out), ptr(keep_out), ptr(full), n, hw, c, sp()), "ctl_dropout2d_ex")
        assert np.array_equal(bits(keep_out.cpu().numpy()), bits(keep)) and np.array_equal(bits(out.cpu().numpy()), bits(ref)), (p, "injected")
        assert np.array_equal(bits(full.cpu().numpy()), bits(ref_full))


@pytest.mark.parametrize("n,c,hw", DROP_SHAPES)
def test_dropout2d_dt_rounds_once_in_every_storage_combination(n, c, hw):
    rng = np.random.default_rng(n * 999 + c + hw)
    keep_out = torch.empty(n, c, device=DEV)
    for m in (0, 1, 2, 3):                                    # bit 0: z is bf16, bit 1: out is bf16
        z = _z(n, c, hw, rng, bf16=bool(m & 1))
        z_d = dev(z).to(torch.bfloat16) if m & 1 else dev(z)
        assert np.array_equal(z_d.float().cpu().numpy(), z)
        for p in PS:
            for seed, state in ((2 ** 63 + 11, None), (2 ** 32 + 5, torch.tensor([as_i64(2 ** 64 - 1), 7, 0], dtype=torch.int64, device=DEV)), (None, None)):
                if seed is None:
                    keep = (rng.random((n, c)) < 0.5).astype(np.float32)
                    keep_d, seed = dev(keep), 0
                else:
                    keep = _keep_ref(seed if state is None else ref_rng.state_seed(2 ** 64 - 1, 7, seed), n, c, p)
                    keep_d = None
                ref, _ = ref_mask.dropout2d(z, keep, p, bf16_in=bool(m & 1), bf16_out=bool(m & 2))
                out = torch.full((n, hw, c), NAN, device=DEV, dtype=torch.bfloat16 if m & 2 else torch.float32)
                keep_out.fill_(NAN)
                check(lib.ctl_dropout2d_dt(ptr(z_d), ptr(keep_d), seed, ptr(state), p, ptr(out), ptr(keep_out), n, hw, c, m, sp()), "ctl_dropout2d_dt")
                got = out.view(torch.int16).cpu().numpy() if m & 2 else out.cpu().numpy()
                assert np.array_equal(bits(got), bits(ref)), (m, p, seed)
                assert np.array_equal(bits(keep_out.cpu().numpy()), bits(keep)), (m, p, seed)


def test_dropout2d_refusals():
    z = torch.zeros(2, 4, 8, device=DEV)
    o, k = torch.empty_like(z), torch.empty(2, 8, device=DEV)
    for p in (1.0, -0.1):
        with pytest.raises(CtlError):
            check(lib.ctl_dropout2d(ptr(z), None, 0, p, ptr(o), ptr(k), 2, 4, 8, sp()))
    with pytest.raises(CtlError):
        check(lib.ctl_dropout2d(ptr(z), None, 0, 0.5, ptr(o), ptr(k), 2, 4, 12, sp()))
    with pytest.raises(CtlError):          # no output
        check(lib.ctl_dropout2d_ex(ptr(z), None, 0, None, 0.5, None, ptr(k), ptr(o), 2, 4, 8, sp()))


# ================================================================================================ noise + clamp
def _noise_clamp(x_d, noise_d, seed, sigma, lo, hi):
    out = torch.full((x_d.numel() + 8,), NAN, device=DEV)
    check(lib.ctl_noise_clamp(ptr(x_d), ptr(noise_d), seed, sigma, lo, hi, ptr(out), x_d.numel(), sp()), "ctl_noise_clamp")
    got = out.cpu().numpy()
    assert np.isnan(got[x_d.numel():]).all()
    return got[:x_d.numel()]


@pytest.mark.parametrize("count", [1, 255, 257, GRID_CAP_ITEMS + 5])
def test_noise_clamp_injected_noise_is_exact(count):
    rng = np.random.default_rng(count)
    x = rng.random(count, dtype=np.float32)
    noise = (0.05 * rng.standard_normal(count)).astype(np.float32)
    q = np.arange(count)
    # sums that land exactly on a bound, just inside and just outside it
    x[q % 5 == 0], noise[q % 5 == 0] = 0.25, -0.25
    x[q % 5 == 1], noise[q % 5 == 1] = 0.75, 0.25
    noise[q % 7 == 2] = 1.0 - x[q % 7 == 2]
    x[q % 11 == 3], noise[q % 11 == 3] = 0.0, -0.0
    x_d, noise_d = dev(x), dev(noise)
    for lo, hi in ((0.0, 1.0), (0.25, 0.75), (0.5, 0.5), (-1.0, 0.0)):
        got = _noise_clamp(x_d, noise_d, 0, 0.05, lo, hi)
        ref = ref_io.noise_clamp(x, noise, lo, hi)
        assert np.array_equal(bits(got), bits(ref)), (lo, hi)
        assert (got >= np.float32(lo)).all() and (got <= np.float32(hi)).all()
    with pytest.raises(CtlError):
        check(lib.ctl_noise_clamp(ptr(x_d), ptr(noise_d), 0, 0.05, 1.0, 0.0, ptr(x_d), count, sp()))       # lo > hi
    with pytest.raises(CtlError):
        check(lib.ctl_noise_clamp(ptr(x_d), ptr(noise_d), 0, 0.05, 0.0, 1.0, ptr(x_d), 0, sp()))


# Maximum error of the device math functions in units in the last place.  No table of these ships with the toolkit's headers; the
# device library is written to the OpenCL full-profile limits (log 3, cos 4; sqrt is correctly rounded in HIP's default mode, 3 is the
# profile's limit), which are at or above the 1 to 2 ulp HIP publishes for logf, sqrtf and cosf.
ULP_LOG, ULP_SQRT, ULP_COS = 3.0, 3.0, 4.0
U = 2.0 ** -24          # half an ulp, relative


@pytest.mark.parametrize("seed,sigma,count", [(0, 0.05, 257), (3, 0.05, GRID_CAP_ITEMS + 5), (2 ** 63 + 9, 0.05, 4099), (2 ** 64 - 1, 2.0, 4099)])
def test_noise_clamp_device_noise_within_the_derived_bound(seed, sigma, count):
    """out = clamp(x + nz) with nz = (sigma * sqrtf(-2 logf(u1))) * cosf(fl(2 pi) * u2) in fp32; u1 and u2 are exact from the
    reference, and clamping is 1-Lipschitz, so |out - clamp(x + nz64)| <= |fl(x + nz) - (x + nz64)| with nz64 the float64 value.

    Per element, with r = sqrt(-2 ln u1) <= sqrt(2 * 24 * ln 2) = 5.77, t = cos(2 pi u2), ulp = 2^-23 relative:
      radius   logf is off by ULP_LOG ulp relative, the factor -2 is exact, the square root halves a relative error and adds its own:
               |r32 - r| <= r * (ULP_LOG / 2 + ULP_SQRT) * 2^-23
      angle    fl(2 pi) differs from 2 pi by 1.75e-7 and u2 < 1; the fp32 product fl(2 pi) * u2 < 8 rounds by at most 2^-22; cos is
               1-Lipschitz and cosf adds ULP_COS ulp of a result <= 1:      |t32 - t| <= 1.75e-7 + 2^-22 + ULP_COS * 2^-23
      products sigma * r32 and (sigma r32) * t32 round once each:           relative 2 * 2^-24
      sum      x + nz rounds once (no contraction: the kernel adds with __fadd_rn): one ulp of the sum, 2^-23 * |x + nz|
    First order:  sigma * r * |t| * ((ULP_LOG / 2 + ULP_SQRT + 1) * 2^-23) + sigma * r * (1.75e-7 + 2^-22 + ULP_COS * 2^-23) + 2^-23 * |x + nz|;
    the second-order terms are below 1e-6 of that and are covered by the factor 1 + 1e-5.  The bound is evaluated per element; its
    largest value is 4.8e-7 at sigma = 0.05 and 1.25e-5 at sigma = 2.  Measured on MI355X: largest error 1.03e-7 at sigma = 0.05 and
    2.25e-6 at sigma = 2, at most 0.47 of the element's bound."""
    rng = np.random.default_rng(count)
    x = rng.random(count, dtype=np.float32)
    x[::5] = 0.5
    idx = np.arange(count, dtype=np.uint64)
    nz, r, t = ref_rng.normal_f64(seed, idx, sigma)
    s = float(np.float32(sigma))
    nz = nz * (s / sigma)
    exact = x.astype(np.float64) + nz
    bound = (s * r * np.abs(t) * (ULP_LOG / 2 + ULP_SQRT + 1) * 2 * U + s * r * (1.75e-7 + 4 * U + ULP_COS * 2 * U) + 2 * U * np.abs(exact)) * (1 + 1e-5)
    x_d = dev(x)
    a = _noise_clamp(x_d, None, seed, sigma, 0.0, 1.0)
    wide = _noise_clamp(x_d, None, seed, sigma, -1e30, 1e30)          # (nothing clamps: the sum itself)
    err_wide = np.abs(wide.astype(np.float64) - exact)
    err = np.abs(a.astype(np.float64) - np.clip(exact, 0.0, 1.0))
    print(f"device noise sigma={sigma} count={count}: max |out - ref| = {err_wide.max():.3e} (clamped: {err.max():.3e}), "
          f"largest bound = {bound.max():.3e}, max error / bound = {(err_wide / bound).max():.3f}")
    assert (err_wide <= bound).all() and (err <= bound).all()
    assert (a >= 0).all() and (a <= 1).all()
    assert np.array_equal(bits(a), bits(_noise_clamp(x_d, None, seed, sigma, 0.0, 1.0)))          # identical bits on every call
