"""Cubic-spline resampling of the batch augmenter on the device (ops.aug_spline_coeffs, ops.aug_warp(interp="cubic"),
augment.BatchAugmenter(interp="cubic")) against scipy.ndimage in fp64 fed the same fp32 parameter values.  The oracle is never the
device code.

Bounds (from the number formats, not from what the kernels give).  For a plane v let r = spline_filter1d(v) along the rows' direction (the
stage the device stores as fp32) and c = spline_filter(v, order=3, mode='reflect').
  coefficients  |device - c| <= 2 * 2^-24 * (3 max|r| + max|c|): the fp32 rounding of the row stage (2^-24 max|r|) passes the column filter,
          whose gain sum |h[k]| is 3, the stored coefficient adds its own rounding 2^-24 max|c|; the factor 2 is the margin.
  image   2 * delta * g + 2 * 2^-24 * (3 max|r| + 2 max|c|) per pixel: delta = 1e-3 px is the coordinate bound of tests/test_aug_gpu.py, g the
          largest |first difference| of c along rows plus the largest along columns over the 6x6 coefficient block around floor(s) (the
          spline's gradient is a convex combination of those differences); the second term is the coefficient bound (the B-spline weights
          are a convex combination) plus the rounding of the stored result.  Pixels whose fp64 s lies within delta of the inside / outside
          boundary (s = -0.5 or side - 0.5 on an axis) are left out; farther outside, image and label are exactly 0.
  label   equal to the oracle wherever, for every class, |value_k - 0.5| exceeds that class's image bound and s is at least delta from the
          boundary; at most 1 % of a sample's pixels may be left out.
  end to end, after the min-max rescale: (B + 3 Bmax) / (mx - mn) + 4 * 2^-24, the form of tests/test_aug_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view
from scipy import ndimage

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, augment, ops
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter

pytestmark = pytest.mark.gpu

DELTA = 1e-3
EPS24 = 2.0 ** -24
N = 3
K = 4                                       # blobs() draws the labels 0..3
SHAPES = [((37, 53), (30, 41)), ((64, 80), (64, 80)), ((224, 224), (192, 192))]
POLICY = "ACDC_affine_elastic_intensity"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- inputs (the generators of test_aug_gpu.py)
def smooth(n, hp, wp, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:hp, 0:wp]
    out = np.zeros((n, 1, hp, wp))
    for b in range(n):
        for _ in range(5):
            cy, cx, s, a = rng.uniform(0, hp), rng.uniform(0, wp), rng.uniform(0.08, 0.3) * hp, rng.uniform(0.3, 1.0)
            out[b, 0] += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
        out[b, 0] += 0.1 * np.sin(x / wp * 6.0 + b) - 0.2
    return out.astype(np.float32)


def checker(n, hp, wp, seed):
    y, x = np.mgrid[0:hp, 0:wp]
    return np.stack([(((y + b) // 3 + x // 3) % 2).astype(np.float32)[None] for b in range(n)])


def noise_img(n, hp, wp, seed):
    return np.random.default_rng(seed).random((n, 1, hp, wp), dtype=np.float32)


IMAGES = {"smooth": smooth, "checker": checker, "noise": noise_img}


def blobs(n, hp, wp, seed):
    rng = np.random.default_rng(100 + seed)
    y, x = np.mgrid[0:hp, 0:wp]
    lab = np.zeros((n, hp, wp), dtype=np.int64)
    for b in range(n):
        for c in (1, 2, 3, 1, 2):
            cy, cx, r = rng.uniform(0.2, 0.8) * hp, rng.uniform(0.2, 0.8) * wp, rng.uniform(0.05, 0.25) * min(hp, wp)
            lab[b][(y - cy) ** 2 + (x - cx) ** 2 < r * r] = c
        lab[b, 0, :] = 3          # labels on the very edge, so that a pulled-in border shows
        lab[b, :, -1] = 2
    return lab


@functools.lru_cache(maxsize=None)
def acdc_params(hp, wp, crop, seed=5, n=N):
    """(matrix, intensity, field) from the ACDC policy ranges, elastic on for every sample; read-only, shared by the tests."""
    p = BatchAugmenter(POLICY, crop, seed).draw(n, hp, wp)
    alpha = p["alpha"].numpy().copy()
    alpha[alpha == 0] = np.float32(1.7 * hp)
    u = np.random.default_rng(seed).random((n, 2, hp, wp)) * 2 - 1
    field = augment.elastic_field_host(alpha, p["sigma"].numpy(), hp, wp, noise=u).astype(np.float32)
    out = (p["matrix"].numpy(), p["intensity"].numpy(), field)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- oracle and bounds
def intensity_map(image, intensity, b):
    return np.clip(image[b, 0].astype(np.float64) * float(intensity[b, 0]) + float(intensity[b, 1]), image[b, 0].min(), image[b, 0].max())


def spline_ref(v):
    """(r, c): the row-filtered plane and the coefficients of v in fp64."""
    v = np.asarray(v, dtype=np.float64)
    return ndimage.spline_filter1d(v, order=3, axis=1, mode="reflect"), ndimage.spline_filter(v, order=3, mode="reflect", output=np.float64)


def coeff_bound(r, c):
    return 2 * EPS24 * (3 * np.abs(r).max() + np.abs(c).max())


def value_bound(r, c, s, delta=DELTA):
    """The per-pixel image bound [hc,wc] of a plane with row stage r and coefficients c at the fp64 source coordinates s [2,hc,wc]."""
    hp, wp = c.shape
    cp = np.pad(c, 4, mode="symmetric")
    # max |row difference| / |column difference| inside the 6x6 block whose first tap is (i0 - 2, j0 - 2): padded index (i0 + 2, j0 + 2)
    gr = sliding_window_view(np.abs(np.diff(cp, axis=0)), (5, 6)).max(axis=(2, 3))
    gc = sliding_window_view(np.abs(np.diff(cp, axis=1)), (6, 5)).max(axis=(2, 3))
    i0 = np.clip(np.floor(s[0]), -1, hp - 1).astype(np.int64) + 2
    j0 = np.clip(np.floor(s[1]), -1, wp - 1).astype(np.int64) + 2
    return 2 * delta * (gr[i0, j0] + gc[i0, j0]) + 2 * EPS24 * (3 * np.abs(r).max() + 2 * np.abs(c).max())


def boundary_masks(s, hp, wp, delta=DELTA):
    """(inside, clear) [n,hc,wc]: where a value is read, and where s is at least delta from the inside / outside boundary."""
    lim = np.array([hp, wp], dtype=np.float64).reshape(1, 2, 1, 1)
    inside = ((s >= -0.5) & (s <= lim - 0.5)).all(axis=1)
    clear = ((np.abs(s + 0.5) >= delta) & (np.abs(s - lim + 0.5) >= delta)).all(axis=1)
    return inside, clear


def cubic_oracle(image, label, matrix, intensity, crop, field, n_class=K):
    """scipy directly (not augment.warp_host): image [n,hc,wc], per-class values [n,K,hc,wc], labels, per-pixel image bound, per-class
    bounds, the fp64 source coordinates."""
    n, _, hp, wp = image.shape
    s = augment.source_coords(matrix, hp, wp, crop[0], crop[1], field)
    inside, _ = boundary_masks(s, hp, wp)
    img, bound = np.zeros((n,) + tuple(crop)), np.zeros((n,) + tuple(crop))
    val, vbound = np.zeros((n, n_class) + tuple(crop)), np.zeros((n, n_class) + tuple(crop))
    lab = np.zeros((n,) + tuple(crop), dtype=np.int64)
    for b in range(n):
        v = intensity_map(image, intensity, b)
        img[b] = np.where(inside[b], ndimage.map_coordinates(v, s[b], order=3, mode="reflect"), 0.0)
        bound[b] = value_bound(*spline_ref(v), s[b])
        for k in range(n_class):
            ind = (label[b] == k).astype(np.float64)
            val[b, k] = ndimage.map_coordinates(ind, s[b], order=3, mode="reflect")
            vbound[b, k] = value_bound(*spline_ref(ind), s[b])
            lab[b][inside[b] & (val[b, k] >= 0.5)] = k
    return img, val, lab, bound, vbound, s


def check_cubic(image, label, matrix, intensity, crop, field, what, n_class=K):
    n, _, hp, wp = image.shape
    io, lo = ops.aug_warp(dev(image), dev(label), dev(matrix), dev(intensity), crop, field=None if field is None else dev(field),
                          interp="cubic", n_class=n_class)
    got_i, got_l = io.cpu().numpy()[:, 0].astype(np.float64), lo.cpu().numpy()
    img, val, lab, bound, vbound, s = cubic_oracle(image, label, matrix, intensity, crop, field, n_class)
    host_i, host_l = augment.warp_host(image, label, matrix, intensity, crop, field, interp="cubic", n_class=n_class)
    assert np.array_equal(host_i[:, 0], img) and np.array_equal(host_l, lab)          # the host statement is the same oracle
    inside, clear = boundary_masks(s, hp, wp)
    err = np.abs(got_i - img)
    print(f"{what}: image max err {err[clear].max():.3e}, max err / bound {np.max((err / bound)[clear]):.3f}, "
          f"near the boundary {int((~clear).sum())} px, outside {100 * (1 - inside.mean()):.1f} %")
    assert np.all(err[clear] <= bound[clear]), (what, float(np.max((err / bound)[clear])))
    assert np.all(got_i[clear & ~inside] == 0) and np.all(got_l[clear & ~inside] == 0)
    keep = clear & (np.abs(val - 0.5) > vbound).all(axis=1)
    left = 1.0 - keep.reshape(n, -1).mean(axis=1)
    print(f"{what}: label pixels left out per sample, max {100 * left.max():.3f} %")
    assert np.all(left <= 0.01), (what, left)
    assert np.array_equal(got_l[keep], lab[keep]), (what, int((got_l[keep] != lab[keep]).sum()))
    return got_i, got_l, s


# ---------------------------------------------------------------------------------------------- coefficients
COEFF_SHAPES = [(5, 7), (15, 16), (16, 15), (17, 39)] + [s[0] for s in SHAPES]


@pytest.mark.parametrize("shape", COEFF_SHAPES, ids=str)
def test_coeffs_match_spline_filter(shape):
    """One sample per image generator.  (5, 7) is far shorter than the filter's reach of 40; 15 / 16 is where the device changes from
    scipy's recursion (lines under 16 samples, where scipy is not the exact inverse) to the reflected FIR, whose reflection folds
    several times up to 39 samples."""
    hp, wp = shape
    image = np.concatenate([IMAGES[k](1, hp, wp, 3) for k in sorted(IMAGES)])
    label = blobs(N, hp, wp, 3)
    intensity = np.float32([[1.0, 0.0], [1.2, 0.1], [0.8, -0.1]])
    got = ops.aug_spline_coeffs(dev(image), dev(label), dev(intensity), n_class=K).cpu().numpy().astype(np.float64)
    assert got.shape == (N, 1 + K, hp, wp)
    for b in range(N):
        planes = [intensity_map(image, intensity, b)] + [(label[b] == k).astype(np.float64) for k in range(K)]
        for pl, v in enumerate(planes):
            r, c = spline_ref(v)
            err = np.abs(got[b, pl] - c).max()
            print(f"{shape} sample {b} plane {pl}: max err {err:.3e}, bound {coeff_bound(r, c):.3e}")
            assert err <= coeff_bound(r, c), (shape, b, pl, err)
    alone = ops.aug_spline_coeffs(dev(image)).cpu().numpy().astype(np.float64)        # the image alone, intensity (1, 0)
    assert alone.shape == (N, 1, hp, wp)
    for b in range(N):
        r, c = spline_ref(image[b, 0])
        assert np.abs(alone[b, 0] - c).max() <= coeff_bound(r, c)


# ---------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("kind", sorted(IMAGES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_warp_cubic_matches_scipy(shape, kind):
    (hp, wp), crop = shape
    image, label = IMAGES[kind](N, hp, wp, 3), blobs(N, hp, wp, 3)
    matrix, intensity, field = acdc_params(hp, wp, crop)
    check_cubic(image, label, matrix, intensity, crop, field, f"{kind} {shape} elastic")
    check_cubic(image, label, matrix, intensity, crop, None, f"{kind} {shape} affine")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identity_reproduces_the_input(shape):
    (hp, wp), _ = shape
    image, label = noise_img(N, hp, wp, 4), blobs(N, hp, wp, 4)
    matrix = np.tile(np.float32([[1, 0, 0], [0, 1, 0]]), (N, 1, 1))
    intensity = np.tile(np.float32([[1, 0]]), (N, 1))
    io, lo = ops.aug_warp(dev(image), dev(label), dev(matrix), dev(intensity), (hp, wp), interp="cubic", n_class=K)
    got = io.cpu().numpy().astype(np.float64)
    for b in range(N):
        err = np.abs(got[b, 0] - image[b, 0]).max()
        print(f"identity {shape} sample {b}: max err {err:.3e}")
        assert err <= coeff_bound(*spline_ref(image[b, 0]))
    assert np.array_equal(lo.cpu().numpy(), label)


def test_constant_plane_stays_constant():
    (hp, wp), crop = SHAPES[0]
    matrix, intensity, field = acdc_params(hp, wp, crop)
    image = np.full((N, 1, hp, wp), 3.0, dtype=np.float32)
    label = np.full((N, hp, wp), 2, dtype=np.int64)
    plain = np.tile(np.float32([[1, 0]]), (N, 1))
    io, lo = ops.aug_warp(dev(image), dev(label), dev(matrix), dev(plain), crop, field=dev(field), interp="cubic", n_class=K)
    inside, clear = boundary_masks(augment.source_coords(matrix, hp, wp, crop[0], crop[1], field), hp, wp)
    got_i, got_l = io.cpu().numpy()[:, 0], lo.cpu().numpy()
    assert 0.05 < inside.mean() < 1.0                                # both sides of the boundary are in view
    assert np.all(got_i[clear & inside] == 3.0) and np.all(got_l[clear & inside] == 2)
    assert np.all(got_i[clear & ~inside] == 0.0) and np.all(got_l[clear & ~inside] == 0)
    assert set(np.unique(got_i)) <= {0.0, 3.0} and set(np.unique(got_l)) <= {0, 2}


def test_labels_are_a_subset_and_classes_beyond_n_class_vanish():
    (hp, wp), crop = SHAPES[2]
    matrix, intensity, field = acdc_params(hp, wp, crop)
    image, label = smooth(N, hp, wp, 6), blobs(N, hp, wp, 6)
    label[1][label[1] == 1] = 7                                       # a value at or above n_class belongs to no class
    label[2][label[2] == 2] = -1
    args = (dev(image), dev(label), dev(matrix), dev(intensity), crop)
    _, lo = ops.aug_warp(*args, field=dev(field), interp="cubic", n_class=K)
    lo = lo.cpu().numpy()
    for b in range(N):
        assert set(np.unique(lo[b])) <= (set(np.unique(label[b])) & set(range(K))) | {0}, b
    assert {1, 2, 3} <= set(np.unique(lo[0])) and 7 not in lo and -1 not in lo
    _, lo3 = ops.aug_warp(*args, field=dev(field), interp="cubic", n_class=3)
    lo3 = lo3.cpu().numpy()
    assert set(np.unique(lo3)) <= {0, 1, 2} and (lo == 3).sum() > 0
    want = augment.warp_host(image, label, matrix, intensity, crop, field, interp="cubic", n_class=3)[1]
    assert (lo3 != want).mean() <= 0.01


# ---------------------------------------------------------------------------------------------- plumbing
def _batch(n, hp, wp, seed):
    return dev(smooth(n, hp, wp, seed)), dev(blobs(n, hp, wp, seed))


@pytest.mark.parametrize("policy", [POLICY, "ACDC_affine_intensity"])
def test_apply_cubic_equals_the_chained_ops_bit_for_bit(policy):
    n, hp, wp, crop = 4, 224, 224, (192, 192)
    image, label = _batch(n, hp, wp, 9)
    aug = BatchAugmenter(policy, crop, 4, interp="cubic", num_classes=K)
    p = aug.upload(aug.draw(n, hp, wp), "cuda")
    io, lo = aug.apply(image, label, p)
    field = None if p["alpha"] is None else ops.aug_elastic_field(n, hp, wp, p["alpha"], p["sigma"], p["seed"])
    w, l2 = ops.aug_warp(image, label, p["matrix"], p["intensity"], crop, field=field, interp="cubic", n_class=K)
    assert torch.equal(io, ops.rescale_intensity(w, 0.0, 1.0)) and torch.equal(lo, l2)
    again = aug.apply(image, label, p)
    assert torch.equal(io, again[0]) and torch.equal(lo, again[1])        # the same bits on every call
    assert tuple(io.shape) == (n, 1) + crop and io.dtype == torch.float32 and tuple(lo.shape) == (n,) + crop and lo.dtype == torch.int64
    out = (torch.empty_like(io), torch.empty_like(lo))
    got = aug.apply(image, label, p, out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], io) and torch.equal(out[1], lo)
    linear = BatchAugmenter(policy, crop, 4).apply(image, label, p)
    assert not torch.equal(linear[0], io)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_apply_cubic_matches_apply_host(shape):
    (hp, wp), crop = shape
    image, label = _batch(N, hp, wp, 10)
    aug = BatchAugmenter(POLICY, crop, 6, interp="cubic", num_classes=K)
    p = aug.draw(N, hp, wp)
    pd = aug.upload(p, "cuda")
    io, lo = aug.apply(image, label, pd)
    # the device's own fp32 displacement goes to the oracle, so that both resample at the same place (the field has its own tests)
    field = None if p["alpha"] is None else ops.aug_elastic_field(N, hp, wp, pd["alpha"], pd["sigma"], pd["seed"]).cpu().numpy()
    img_h, lab_h = image.cpu().numpy(), label.cpu().numpy()
    want_i, want_l = augment.apply_host(img_h, lab_h, p, field=field, interp="cubic", n_class=K)
    matrix, intensity = p["matrix"].numpy(), p["intensity"].numpy()
    warped, val, lab, bound, vbound, s = cubic_oracle(img_h, lab_h, matrix, intensity, crop, field)
    assert np.array_equal(want_l, lab)
    inside, clear = boundary_masks(s, hp, wp)
    mn, mx = warped.min(axis=(1, 2), keepdims=True), warped.max(axis=(1, 2), keepdims=True)
    # a pixel within delta of the boundary may be read as 0 or as its value: neither may move the plane's minimum or maximum
    for b in range(N):
        near = ~clear[b]
        both = np.concatenate([warped[b][near], np.zeros(int(near.sum()))])
        rest = warped[b][clear[b]]
        assert both.size == 0 or (both.min() >= rest.min() and both.max() <= rest.max()), (shape, b)
    full = (bound + 3 * bound.max(axis=(1, 2), keepdims=True)) / (mx - mn) + 4 * EPS24
    err = np.abs(io.cpu().numpy()[:, 0].astype(np.float64) - want_i[:, 0])
    print(f"end to end {shape}: max err {err[clear].max():.3e}, max err / bound {np.max((err / full)[clear]):.3f}")
    assert np.all(err[clear] <= full[clear])
    keep = clear & (np.abs(val - 0.5) > vbound).all(axis=1)
    left = 1.0 - keep.reshape(N, -1).mean(axis=1)
    print(f"end to end {shape}: label pixels left out, max {100 * left.max():.3f} %")
    assert np.all(left <= 0.01)
    assert np.array_equal(lo.cpu().numpy()[keep], want_l[keep])


def test_graph_replay_equals_eager():
    n, hp, wp, crop = 4, 224, 224, (192, 192)
    aug = BatchAugmenter(POLICY, crop, 3, interp="cubic", num_classes=K)
    image, label = _batch(n, hp, wp, 13)
    p = aug.upload(aug.draw(n, hp, wp), "cuda")
    s_image, s_label = image.clone(), label.clone()
    s_p = {k: (v.clone() if isinstance(v, torch.Tensor) and v.is_cuda else v) for k, v in p.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.apply(s_image, s_label, s_p)                          # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_image, g_label = aug.apply(s_image, s_label, s_p)
    for seed in (14, 15):
        image, label = _batch(n, hp, wp, seed)
        p = aug.upload(aug.draw(n, hp, wp), "cuda")
        s_image.copy_(image)
        s_label.copy_(label)
        for k in augment.DEVICE_KEYS:
            s_p[k].copy_(p[k])
        graph.replay()
        torch.cuda.synchronize()
        want = aug.apply(image, label, p)
        assert torch.equal(g_image, want[0]) and torch.equal(g_label, want[1])


@pytest.mark.parametrize("n", [1, 16])
def test_launch_count_does_not_depend_on_n(n):
    hp, wp, crop = 64, 80, (64, 80)
    image, label = _batch(n, hp, wp, 16)
    for policy, launches in ((POLICY, 8), ("ACDC_affine_intensity", 6)):
        aug = BatchAugmenter(policy, crop, 1, interp="cubic", num_classes=K)
        p = aug.upload(aug.draw(n, hp, wp), "cuda")
        before = _ffi.lib.ctl_launch_count()
        aug.apply(image, label, p)
        assert _ffi.lib.ctl_launch_count() - before == launches, (policy, n)
    before = _ffi.lib.ctl_launch_count()
    ops.aug_spline_coeffs(image, label, p["intensity"], n_class=K)
    assert _ffi.lib.ctl_launch_count() - before == 3


def test_linear_is_the_unchanged_warp_bit_for_bit():
    n, hp, wp, crop = 4, 224, 224, (192, 192)
    image, label = _batch(n, hp, wp, 17)
    aug = BatchAugmenter(POLICY, crop, 5, interp="linear")
    assert aug.interp == "linear" == BatchAugmenter(POLICY, crop, 5).interp
    p = aug.upload(aug.draw(n, hp, wp), "cuda")
    field = ops.aug_elastic_field(n, hp, wp, p["alpha"], p["sigma"], p["seed"])
    w, l2 = ops.aug_warp(image, label, p["matrix"], p["intensity"], crop, field=field)          # the call as it was before interp existed
    w2, l3 = ops.aug_warp(image, label, p["matrix"], p["intensity"], crop, field=field, interp="linear")
    assert torch.equal(w, w2) and torch.equal(l2, l3)
    before = _ffi.lib.ctl_launch_count()
    io, lo = aug.apply(image, label, p)
    assert _ffi.lib.ctl_launch_count() - before == 6
    assert torch.equal(io, ops.rescale_intensity(w, 0.0, 1.0)) and torch.equal(lo, l2)
    with pytest.raises(ValueError, match="interp"):
        ops.aug_warp(image, label, p["matrix"], p["intensity"], crop, interp="nearest")
    with pytest.raises(ValueError, match="n_class"):
        ops.aug_warp(image, label, p["matrix"], p["intensity"], crop, interp="cubic")
    with pytest.raises(ValueError, match="n_class"):
        ops.aug_warp(image, label, p["matrix"], p["intensity"], crop, interp="cubic", n_class=17)
