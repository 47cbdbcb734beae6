"""The I/O kernels of csrc/ctl_io.hip (ctl_confusion_hist, ctl_rescale_intensity, ctl_crop_or_pad) through the C ABI against the host
restatement of their header contract in oracle/ref_io.py, which tests/test_ref_mask_rng_io_cpu.py ties to the upstream-recorded
results of tests/golden/io_cases.pt.  Integer results are compared as integers, float results bit for bit.  (ctl_noise_clamp, which
draws from the counter-hash RNG, is in tests/test_rng_exact_gpu.py.)"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check, CtlError  # noqa: E402
from oracle import ref_io  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 256


def sp():
    return ops.stream_ptr()


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ================================================================================================ confusion histogram
def _hist(lt, lp, n_class, hist):
    check(lib.ctl_confusion_hist(ptr(lt), ptr(lp), lt.numel(), n_class, ptr(hist), sp()), "ctl_confusion_hist")


@pytest.mark.parametrize("n_class", [1, 2, 4, 16])
def test_confusion_hist_counts_exactly(n_class):
    """counts below, at and above one block, and 300001 above the 1024-block grid cap; true labels include -1, n_class and a large int64
    (ignored), predictions include values >= n_class and 255 (ignored); the histogram accumulates over calls"""
    rng = np.random.default_rng(n_class)
    for count in (1, 255, 257, 300001):
        lt = rng.integers(-1, n_class + 1, count).astype(np.int64)
        lp = rng.integers(0, min(n_class + 2, 256), count).astype(np.uint8)
        if count > 1:
            q = np.arange(count)
            lt[q % 13 == 5] = 2 ** 40 + 1
            lt[q % 17 == 6] = -2 ** 62
            lp[q % 19 == 7] = 255
            lt[-1], lp[-1] = n_class - 1, n_class - 1
        else:
            lt[0], lp[0] = n_class - 1, 0
        hist = torch.zeros(n_class * n_class + GUARD, dtype=torch.int64, device=DEV)
        lt_d, lp_d = dev(lt), dev(lp)
        _hist(lt_d, lp_d, n_class, hist)
        ref = ref_io.confusion(lt, lp, n_class)
        got = hist.cpu().numpy()
        assert np.array_equal(got[:n_class * n_class].reshape(n_class, n_class), ref), count
        assert ref.sum() > 0 and not got[n_class * n_class:].any()
        # a second batch into the non-zero histogram
        lt2, lp2 = lt[::-1].copy(), np.roll(lp, 3)
        _hist(dev(lt2), dev(lp2), n_class, hist)
        ref2 = ref_io.confusion(lt2, lp2, n_class, ref)
        assert np.array_equal(hist.cpu().numpy()[:n_class * n_class].reshape(n_class, n_class), ref2), count
        assert ref2.sum() == ref.sum() + ref_io.confusion(lt2, lp2, n_class).sum()
    # every element in one bin, more elements than one grid pass
    count = 300001
    t, p = n_class - 1, n_class // 2
    hist = torch.zeros(n_class * n_class, dtype=torch.int64, device=DEV)
    _hist(torch.full((count,), t, dtype=torch.int64, device=DEV), torch.full((count,), p, dtype=torch.uint8, device=DEV), n_class, hist)
    ref = np.zeros((n_class, n_class), dtype=np.int64)
    ref[t, p] = count
    assert np.array_equal(hist.cpu().numpy().reshape(n_class, n_class), ref)
    assert np.array_equal(ref, ref_io.confusion(np.full(count, t), np.full(count, p), n_class))


def test_confusion_hist_refusals():
    lt, lp = torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV)
    hist = torch.zeros(17 * 17, dtype=torch.int64, device=DEV)
    for count, n_class in ((8, 17), (0, 4), (8, 0), (-1, 4)):
        with pytest.raises(CtlError):
            check(lib.ctl_confusion_hist(ptr(lt), ptr(lp), count, n_class, ptr(hist), sp()))
    with pytest.raises(CtlError):
        check(lib.ctl_confusion_hist(ptr(lt), ptr(lp), 8, 4, None, sp()))
    assert not hist.any()


# ================================================================================================ min-max rescale
RS_BLOCK, RS_BLOCKS_PER_PLANE = 256, 64          # one pass of a plane's 64 blocks covers 64 * 256 elements
PASS = RS_BLOCK * RS_BLOCKS_PER_PLANE


def _rescale(x, new_min, new_max, eps):
    planes, pe = x.shape
    ws_floats = lib.ctl_rescale_intensity_ws_floats(planes)
    assert ws_floats >= planes * RS_BLOCKS_PER_PLANE * 2
    ws = torch.full((ws_floats + GUARD,), NAN, device=DEV)
    out = torch.full((planes * pe + GUARD,), NAN, device=DEV)
    check(lib.ctl_rescale_intensity(ptr(dev(x)), ptr(out), ptr(ws), planes, pe, new_min, new_max, eps, sp()), "ctl_rescale_intensity")
    got = out.cpu().numpy()
    assert np.isnan(got[planes * pe:]).all() and bool(torch.isnan(ws[ws_floats:]).all())          # guards untouched
    return got[:planes * pe].reshape(planes, pe)


@pytest.mark.parametrize("plane_elems", [1, 63, 256, PASS - 1, PASS + 1, 100003])
@pytest.mark.parametrize("planes", [1, 3])
def test_rescale_intensity_is_bit_equal(planes, plane_elems):
    """((x - mn) / ((mx - mn) + eps)) * (new_max - new_min) + new_min per plane, one rounding per operation, with the extrema at the
    edges of the reduction (first / last lane of a block, first / last element of a grid pass, last element of the plane).  NaN
    inputs are out of scope: the kernel's fminf / fmaxf drop a NaN where torch.min / max propagate it."""
    rng = np.random.default_rng(planes * 1000003 + plane_elems)
    shape = (planes, plane_elems)
    x = rng.random(shape, dtype=np.float32)
    cases = [("random", x, 0.0, 1.0, 1e-20), ("eps", x * 100 - 30, -1.0, 1.0, 1e-3), ("new_min > new_max", x, 1.0, -0.5, 1e-20),
             ("constant", np.full(shape, 3.5, dtype=np.float32), 0.25, 1.0, 1e-20),
             ("constant zero", np.zeros(shape, dtype=np.float32), 0.0, 1.0, 1e-20),
             ("negative only", -x - 0.5, 0.0, 1.0, 1e-20)]
    for idx in sorted({i for i in (0, 255, 256, PASS - 1, PASS, plane_elems - 1) if i < plane_elems}):
        lo, hi = x.copy(), x.copy()
        lo[:, idx], hi[:, idx] = -7.5, 9.25
        both = x.copy()
        both[:, idx] = 9.25
        both[:, plane_elems - 1 - idx] = -7.5 if plane_elems - 1 - idx != idx else 9.25
        cases += [(f"min at {idx}", lo, 0.0, 1.0, 1e-20), (f"max at {idx}", hi, 0.0, 1.0, 1e-20), (f"max at {idx}, min mirrored", both, 0.0, 255.0, 1e-20)]
    for what, xs, new_min, new_max, eps in cases:
        xs = np.ascontiguousarray(xs, dtype=np.float32)
        ref = ref_io.rescale(xs, new_min, new_max, eps)
        got = _rescale(xs, new_min, new_max, eps)
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (what, float(np.abs(got - ref).max()))
        if what.startswith("constant"):
            assert (got == np.float32(new_min)).all()
        if what.startswith(("min at", "max at")) and plane_elems > 1:
            idx = int(what.split()[2].rstrip(","))
            assert (got[:, idx] == (0.0 if what.startswith("min") else new_max)).all()


def test_rescale_intensity_refusals():
    x = torch.zeros(64, device=DEV)
    ws = torch.zeros(lib.ctl_rescale_intensity_ws_floats(1), device=DEV)
    assert lib.ctl_rescale_intensity_ws_floats(0) == 0
    for planes, pe, w in ((0, 64, ws), (1, 0, ws), (1, 64, None)):
        with pytest.raises(CtlError):
            check(lib.ctl_rescale_intensity(ptr(x), ptr(x), ptr(w), planes, pe, 0.0, 1.0, 1e-20, sp()))


# ================================================================================================ crop or pad
SIZES = [(5, 8), (8, 5), (7, 7), (6, 9), (9, 6), (1, 4), (4, 1)]          # odd / even differences in both directions, and no change


def _src(n, h, w, dtype, rng):
    """no element is zero, so a padded zero cannot be mistaken for a copied one"""
    if dtype == np.uint8:
        return rng.integers(1, 256, (n, h, w)).astype(np.uint8)
    if dtype == np.int64:
        a = rng.integers(-2 ** 62, 2 ** 62, (n, h, w)).astype(np.int64)
        return np.where(a == 0, 1, a)
    return (rng.random((n, h, w), dtype=np.float32) + np.float32(0.5)) * np.where(rng.random((n, h, w)) < 0.5, -1, 1).astype(np.float32)


def _crop_or_pad(src, new_h, new_w):
    n, h, w = src.shape
    total = n * new_h * new_w
    dst = torch.from_numpy(np.full(total + GUARD, 0x5A, dtype=np.uint8).repeat(src.dtype.itemsize).view(src.dtype)).to(DEV)
    check(lib.ctl_crop_or_pad(ptr(dev(src)), ptr(dst), src.dtype.itemsize, n, h, w, new_h, new_w, sp()), "ctl_crop_or_pad")
    got = dst.cpu().numpy()
    assert (got[total:].view(np.uint8) == 0x5A).all()
    return got[:total].reshape(n, new_h, new_w)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.int64], ids=["1 byte", "4 bytes", "8 bytes"])
@pytest.mark.parametrize("n", [1, 3])
def test_crop_or_pad_every_parity(n, dtype):
    rng = np.random.default_rng(n * 10 + np.dtype(dtype).itemsize)
    for (h, new_h), (w, new_w) in itertools.product(SIZES, SIZES):
        src = _src(n, h, w, dtype, rng)
        ref = ref_io.crop_or_pad(src, new_h, new_w)
        got = _crop_or_pad(src, new_h, new_w)
        assert got.tobytes() == ref.tobytes(), (h, new_h, w, new_w)
        assert (ref != 0).sum() == n * min(h, new_h) * min(w, new_w)          # the centre window is copied, the rest is zero


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.int64], ids=["1 byte", "4 bytes", "8 bytes"])
def test_crop_or_pad_above_the_grid_cap(dtype):
    """3 x 500 x 520 = 780000 outputs > 2048 blocks * 256: the loop strides; crop along h, pad along w"""
    rng = np.random.default_rng(7)
    src = _src(3, 512, 512, dtype, rng)
    ref = ref_io.crop_or_pad(src, 500, 520)
    assert ref.shape == (3, 500, 520) and not ref[:, :, :4].any() and not ref[:, :, 516:].any() and np.array_equal(ref[:, :, 4:516], src[:, 6:506, :])
    assert _crop_or_pad(src, 500, 520).tobytes() == ref.tobytes()


def test_crop_or_pad_refusals():
    a = torch.zeros(64, dtype=torch.int64, device=DEV)
    for eb, n, h, w, nh, nw in ((2, 1, 4, 4, 4, 4), (3, 1, 4, 4, 4, 4), (16, 1, 2, 2, 2, 2), (4, 0, 4, 4, 4, 4), (4, 1, 4, 4, 0, 4), (4, 1, 4, 4, 4, -1)):
        with pytest.raises(CtlError):
            check(lib.ctl_crop_or_pad(ptr(a), ptr(a), eb, n, h, w, nh, nw, sp()))
