"""Batch augmentation on the device (ops.aug_elastic_field, ops.aug_warp, augment.BatchAugmenter) against scipy in fp64 fed the same
fp32 parameter values.  The oracle is never the device code.

Bounds (from the number formats, not from what the kernels give):
  field   4e-5 * alpha: each pass sums at most 309 non-negative normalised weights times |u| <= 1, so fp32 accumulation loses at most
          (taps + 1) * 2^-24 ~ 1.9e-5 per pass.
  image   2 * delta * r + 4 * 2^-24 * max|v| per pixel, delta = 1e-3 px (fp32 ulp at coordinates of 256..512 is 3.05e-5, at most 8 rounded
          operations: 2.5e-4 px, a 4x margin), r = the value range (after the intensity map, zeros outside the array) of the 3x3 source
          neighbourhood centred on the pixel nearest to the oracle's source coordinate -- the cells a coordinate that is off by delta can
          reach from there.
  label   equal to map_coordinates(order=0, mode='grid-constant') except where the fp64 source coordinate lies within 1e-3 of a rounding
          boundary on either axis; at most 1 % of a sample's pixels may be left out that way.
  end to end, after the min-max rescale (x - mn) / (mx - mn): with B the warp bound of a pixel and Bmax its maximum over the plane (which
          also bounds the error of mn and mx), |error| <= (B + 3 Bmax) / (mx - mn) + 4 * 2^-24.
"""
import numpy as np
import pytest
import torch
from scipy import ndimage

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, augment, ops
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter

pytestmark = pytest.mark.gpu

DELTA = 1e-3
EPS24 = 2.0 ** -24
SHAPES = [((224, 224), (192, 192)), ((256, 256), (256, 256)), ((37, 53), (30, 41)), ((224, 256), (192, 200))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- inputs
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


# ---------------------------------------------------------------------------------------------- bounds
def warp_bound(image, matrix, intensity, crop, field, delta=DELTA):
    """Per-pixel image bound [n,hc,wc] and the fp64 source coordinates.  delta: a scalar or one coordinate tolerance per sample."""
    n, _, hp, wp = image.shape
    s = augment.source_coords(matrix, hp, wp, crop[0], crop[1], field)
    bound = np.zeros((n, crop[0], crop[1]))
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), (n,))
    pad = 4
    for b in range(n):
        v = np.clip(image[b, 0].astype(np.float64) * float(intensity[b, 0]) + float(intensity[b, 1]), image[b, 0].min(), image[b, 0].max())
        vp = np.pad(v, pad)
        r = ndimage.maximum_filter(vp, size=3, mode="constant") - ndimage.minimum_filter(vp, size=3, mode="constant")
        iy = np.clip(np.floor(s[b, 0] + 0.5), -2, hp + 1).astype(np.int64) + pad
        ix = np.clip(np.floor(s[b, 1] + 0.5), -2, wp + 1).astype(np.int64) + pad
        bound[b] = 2 * delta[b] * r[iy, ix] + 4 * EPS24 * np.abs(image[b, 0]).max()
    return bound, s


def label_mask(s, delta=1e-3):
    """True where the label must be exactly equal: farther than delta (1e-3; a scalar or one value per sample) from a rounding boundary
    on both axes.  [n,hc,wc]"""
    t = s + 0.5
    return (np.abs(t - np.round(t)) >= np.reshape(delta, (-1, 1, 1, 1))).all(axis=1)


def check_warp(image, label, matrix, intensity, crop, field=None, exact=False, what=""):
    """Device warp against the scipy oracle; returns the share of left-out label pixels per sample."""
    f_d = None if field is None else dev(field)
    io, lo = ops.aug_warp(dev(image), dev(label), dev(matrix), dev(intensity), crop, field=f_d)
    want_i, want_l = augment.warp_host(image, label, matrix, intensity, crop, field)
    bound, s = warp_bound(image, matrix, intensity, crop, field)
    err = np.abs(io.cpu().numpy()[:, 0].astype(np.float64) - want_i[:, 0])
    print(f"{what}: image max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (what, float(np.max(err / bound)))
    keep = np.ones_like(want_l, dtype=bool) if exact else label_mask(s)
    left = 1.0 - keep.reshape(keep.shape[0], -1).mean(axis=1)
    print(f"{what}: label pixels left out per sample, max {100 * left.max():.3f} %")
    assert np.all(left <= 0.01), (what, left)
    assert np.array_equal(lo.cpu().numpy()[keep], want_l[keep]), what
    return io, lo, want_i, want_l


# ---------------------------------------------------------------------------------------------- field
@pytest.mark.parametrize("shape", [(192, 192), (224, 256), (37, 53)], ids=str)
def test_field_matches_gaussian_filter(shape):
    hp, wp = shape
    sigmas = np.float32([3.0, 14.4, 28.8, 38.4])
    alphas = np.float32([300.0, 1.0, 448.0, 512.0])
    u = (np.random.default_rng(1).random((4, 2, hp, wp), dtype=np.float32) * 2 - 1).astype(np.float32)
    got = ops.aug_elastic_field(4, hp, wp, torch.from_numpy(alphas), torch.from_numpy(sigmas), 0, noise=dev(u)).cpu().numpy()
    for b in range(4):
        for a in range(2):
            want = float(alphas[b]) * ndimage.gaussian_filter(u[b, a].astype(np.float64), sigma=float(sigmas[b]), mode="constant", cval=0.0,
                                                              truncate=4.0)
            err = np.abs(got[b, a] - want).max()
            print(f"{shape} sigma {sigmas[b]} axis {a}: max err {err:.3e} = {err / alphas[b]:.3e} * alpha")
            assert err <= 4e-5 * alphas[b], (shape, b, a, err)
    want_all = augment.elastic_field_host(alphas, sigmas, hp, wp, noise=u)
    assert np.abs(got - want_all).max() <= 4e-5 * alphas.max()


def test_field_zero_alpha_and_zero_sigma():
    u = dev(np.random.default_rng(2).random((3, 2, 40, 72), dtype=np.float32) * 2 - 1)
    out = torch.full((3, 2, 40, 72), 7.0, device="cuda")
    got = ops.aug_elastic_field(3, 40, 72, torch.tensor([0.0, 2.0, 5.0]), torch.tensor([6.0, 0.0, 2.0]), 0, noise=u, out=out)
    assert got is out
    assert torch.count_nonzero(got[0]) == 0                       # alpha 0: zeros without filtering
    assert torch.equal(got[1], 2.0 * u[1])                        # sigma 0: radius 0, the identity
    assert got[2].abs().max() > 0


def test_hash_noise_is_reproducible_keyed_and_uniform():
    n, hp, wp = 16, 256, 256
    one, zero = torch.ones(n), torch.zeros(n)                     # sigma 0 and alpha 1 hand back u itself
    seeds = torch.arange(n, dtype=torch.int64) + 11
    a = ops.aug_elastic_field(n, hp, wp, one, zero, seeds)
    b = ops.aug_elastic_field(n, hp, wp, one, zero, seeds)
    assert torch.equal(a, b)
    c = ops.aug_elastic_field(n, hp, wp, one, zero, seeds + 1)
    assert not torch.equal(a, c)
    same = ops.aug_elastic_field(n, hp, wp, one, zero, 5)         # one seed for all: still keyed by sample and axis
    flat = same.reshape(n * 2, -1)
    assert len({tuple(r[:64].tolist()) for r in flat.cpu()}) == n * 2
    u = a.cpu().numpy().astype(np.float64)
    assert u.min() >= -1 and u.max() < 1
    cnt = u.size
    print(f"hash noise: mean {u.mean():.3e}, var {u.var():.6f} over {cnt} values")
    assert abs(u.mean()) <= 5 * np.sqrt(1 / 3 / cnt)
    assert abs(u.var() - 1 / 3) <= 5 * np.sqrt(4 / 45 / cnt)      # Var((u - mean)^2) of uniform [-1, 1) = 1/5 - 1/9
    assert np.array_equal(u[:3], augment.hash_noise(seeds[:3].numpy(), hp, wp))       # the host states the same generator
    # filtered: the device's field from hash noise against the host's from the same u
    al, sg = torch.full((n,), 400.0), torch.full((n,), 20.0)
    f = ops.aug_elastic_field(n, hp, wp, al, sg, seeds).cpu().numpy()
    want = augment.elastic_field_host(al.numpy()[:2], sg.numpy()[:2], hp, wp, seeds=seeds.numpy()[:2])
    assert np.abs(f[:2] - want).max() <= 4e-5 * 400.0


# ---------------------------------------------------------------------------------------------- warp
def acdc_params(n, hp, wp, crop, seed, elastic_all=True):
    aug = BatchAugmenter("ACDC_affine_elastic_intensity", crop, seed)
    p = aug.draw(n, hp, wp)
    alpha = p["alpha"].numpy().copy()
    if elastic_all:
        alpha[alpha == 0] = np.float32(1.7 * hp)
    u = np.random.default_rng(seed).random((n, 2, hp, wp)) * 2 - 1
    field = augment.elastic_field_host(alpha, p["sigma"].numpy(), hp, wp, noise=u).astype(np.float32)
    return p["matrix"].numpy(), p["intensity"].numpy(), field


@pytest.mark.parametrize("kind", sorted(IMAGES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_warp_matches_scipy(shape, kind):
    (hp, wp), crop = shape
    n = 6
    image, label = IMAGES[kind](n, hp, wp, 3), blobs(n, hp, wp, 3)
    matrix, intensity, field = acdc_params(n, hp, wp, crop, 5)
    check_warp(image, label, matrix, intensity, crop, field, what=f"{kind} {shape} elastic")
    check_warp(image, label, matrix, intensity, crop, None, what=f"{kind} {shape} affine")


@pytest.mark.parametrize("size", [192, 224, 256])
def test_label_left_out_share_over_many_draws(size):
    crop = (192, 192) if size == 224 else (size, size)
    image, label = smooth(10, size, size, 1), blobs(10, size, size, 1)
    for seed in range(2):
        matrix, intensity, field = acdc_params(10, size, size, crop, 40 + seed)
        check_warp(image, label, matrix, intensity, crop, field, what=f"{size} seed {seed}")


def _exact_params(hp, wp):
    flips = [(False, False), (True, False), (False, True), (True, True), (False, False), (False, False)]
    trans = [(0, 0)] * 4 + [(5 / hp, -7 / wp), (-11 / hp, 3 / wp)]
    return augment.compose_matrix(flips, [0.0] * 6, trans, [(1.0, 1.0)] * 6, [0.0] * 6, hp, wp).astype(np.float32)


@pytest.mark.parametrize("shape", [((64, 80), (64, 80)), ((65, 80), (40, 51)), ((224, 224), (192, 192))], ids=str)
def test_identity_flips_and_integer_translations_are_exact(shape):
    (hp, wp), crop = shape
    image, label = noise_img(6, hp, wp, 4), blobs(6, hp, wp, 4)
    matrix = _exact_params(hp, wp)
    intensity = np.tile(np.float32([[1, 0]]), (6, 1))
    io, lo, want_i, want_l = check_warp(image, label, matrix, intensity, crop, None, exact=True, what=f"exact {shape}")
    assert np.array_equal(io.cpu().numpy().astype(np.float64), want_i)
    cy, cx = augment.crop_offsets(hp, wp, *crop)
    assert np.array_equal(lo[0].cpu().numpy(), label[0, cy:cy + crop[0], cx:cx + crop[1]])
    assert np.array_equal(io[0, 0].cpu().numpy(), image[0, 0, cy:cy + crop[0], cx:cx + crop[1]])
    # a translated window: rows + 5, columns - 7, zeros where it leaves the array
    ys, xs = np.arange(crop[0]) + cy + 5, np.arange(crop[1]) + cx - 7
    inside = ((ys >= 0) & (ys < hp))[:, None] & ((xs >= 0) & (xs < wp))[None, :]
    moved = np.where(inside, label[4][np.clip(ys, 0, hp - 1)[:, None], np.clip(xs, 0, wp - 1)[None, :]], 0)
    assert np.array_equal(lo[4].cpu().numpy(), moved)


def test_quarter_turns_are_exact_on_a_square_plane():
    image, label = noise_img(4, 96, 96, 5), blobs(4, 96, 96, 5)
    matrix = augment.compose_matrix([(False, False)] * 4, [0.0] * 4, [(0, 0)] * 4, [(1.0, 1.0)] * 4, [0.0, 90.0, 180.0, 270.0], 96, 96).astype(np.float32)
    intensity = np.tile(np.float32([[1, 0]]), (4, 1))
    io, lo, _, _ = check_warp(image, label, matrix, intensity, (96, 96), None, exact=True, what="quarter turns")
    for b, k in enumerate((0, -1, 2, 1)):
        assert np.array_equal(lo[b].cpu().numpy(), np.rot90(label[b], k))
        assert np.array_equal(io[b, 0].cpu().numpy(), np.rot90(image[b, 0], k))


def test_border_pulled_into_view_is_zero_where_the_oracle_says():
    hp, wp, crop = 128, 160, (128, 160)
    image = noise_img(4, hp, wp, 6) + 1.0                       # strictly positive: a zero in the output is the border
    label = blobs(4, hp, wp, 6) + 1                             # likewise
    matrix = augment.compose_matrix([(False, False)] * 4, [0.0, 0.0, 30.0, 0.0], [(0.25, 0.0), (0.0, -0.3), (0.1, 0.1), (0.0, 0.0)],
                                    [(1.0, 1.0), (1.0, 1.0), (1.5, 1.5), (2.1, 1.8)], [0.0] * 4, hp, wp).astype(np.float32)
    intensity = np.tile(np.float32([[1, 0]]), (4, 1))
    io, lo, want_i, want_l = check_warp(image, label, matrix, intensity, crop, None, what="border")
    got_i, got_l = io.cpu().numpy()[:, 0], lo.cpu().numpy()
    s = augment.source_coords(matrix, hp, wp, *crop)
    # the image turns zero where s passes -1 or the array size; a coordinate within delta of that line may fall on either side
    clear = ((np.abs(s[:, 0] + 1) >= DELTA) & (np.abs(s[:, 0] - hp) >= DELTA) & (np.abs(s[:, 1] + 1) >= DELTA) & (np.abs(s[:, 1] - wp) >= DELTA))
    assert clear.mean() > 0.99
    assert np.array_equal((got_i == 0)[clear], (want_i[:, 0] == 0)[clear])
    keep = label_mask(s)
    assert np.array_equal((got_l == 0)[keep], (want_l == 0)[keep])
    for b in range(4):
        assert 0.1 < (got_l[b] == 0).mean() < 0.9 and 0.1 < (got_i[b] == 0).mean() < 0.9


def test_intensity_map_clamps_to_the_plane_range():
    hp, wp = 64, 64
    image, label = smooth(3, hp, wp, 7), blobs(3, hp, wp, 7)
    matrix = np.tile(np.float32([[1, 0, 0], [0, 1, 0]]), (3, 1, 1))
    intensity = np.float32([[1.2, 0.1], [0.8, -0.1], [1.0, 0.0]])
    io, _, want_i, _ = check_warp(image, label, matrix, intensity, (64, 64), None, exact=True, what="intensity")
    got = io.cpu().numpy()
    for b in range(3):
        assert got[b].max() <= image[b].max() and got[b].min() >= image[b].min()
    assert (got[0] == image[0].max()).sum() > 1 and (got[1] == image[1].min()).sum() >= 1         # the clamp is active
    assert np.array_equal(got[2], image[2])


def test_warp_out_aliasing_and_argument_errors():
    hp, wp, crop = 64, 64, (64, 64)
    image, label = dev(noise_img(2, hp, wp, 8)), dev(blobs(2, hp, wp, 8))
    matrix = dev(np.tile(np.float32([[0, -1, 0], [1, 0, 0]]), (2, 1, 1)))
    intensity = dev(np.tile(np.float32([[1, 0]]), (2, 1)))
    want = ops.aug_warp(image, label, matrix, intensity, crop)
    io, lo = torch.empty_like(image), torch.empty_like(label)
    got = ops.aug_warp(image, label, matrix, intensity, crop, out=(io, lo))
    assert got[0] is io and got[1] is lo and torch.equal(io, want[0]) and torch.equal(lo, want[1])
    keep_i, keep_l = image.clone(), label.clone()
    with pytest.raises(_ffi.CtlError, match="overlaps"):         # an output on top of its input is refused, nothing is written
        ops.aug_warp(image, label, matrix, intensity, crop, out=(image, lo))
    with pytest.raises(_ffi.CtlError, match="overlaps"):
        ops.aug_warp(image, label, matrix, intensity, crop, out=(io, label))
    with pytest.raises(_ffi.CtlError, match="overlaps"):         # the two outputs on top of each other (4- and 8-byte elements)
        ops.aug_warp(image, label, matrix, intensity, crop, out=(lo.view(torch.float32).view(-1)[:io.numel()].view(io.shape), lo))
    fld = torch.zeros(2, 2, hp, wp, device="cuda")
    with pytest.raises(_ffi.CtlError, match="overlaps"):         # an output on top of the displacement field
        ops.aug_warp(image, label, matrix, intensity, crop, field=fld, out=(fld.view(-1)[:io.numel()].view(io.shape), lo))
    u = torch.zeros(2, 2, hp, wp, device="cuda")
    with pytest.raises(_ffi.CtlError, match="overlap"):
        ops.aug_elastic_field(2, hp, wp, 1.0, 2.0, 0, noise=u, out=u)
    assert torch.equal(image, keep_i) and torch.equal(label, keep_l)
    with pytest.raises(ValueError):
        ops.aug_warp(image, label, matrix, intensity, (65, 64))
    with pytest.raises(ValueError):
        ops.aug_warp(image, label.int(), matrix, intensity, crop)
    with pytest.raises(ValueError):
        ops.aug_warp(image, label, matrix[:1], intensity, crop)
    with pytest.raises(ValueError):
        ops.aug_warp(image, label, matrix, intensity, crop, out=(io[:, :, :32], lo))
    with pytest.raises(ValueError):
        ops.aug_elastic_field(2, 513, 64, 1.0, 2.0, 0)
    with pytest.raises(_ffi.CtlError):
        ops.aug_warp(image.cpu(), label, matrix, intensity, crop)


# ---------------------------------------------------------------------------------------------- end to end
def _batch(n, hp, wp, seed):
    return dev(smooth(n, hp, wp, seed)), dev(blobs(n, hp, wp, seed))


@pytest.mark.parametrize("policy", ["ACDC_affine_elastic_intensity", "ACDC_affine_intensity", "no_aug"])
def test_apply_equals_the_chained_ops_bit_for_bit(policy):
    n, hp, wp, crop = 8, 224, 224, (192, 192)
    image, label = _batch(n, hp, wp, 9)
    aug = BatchAugmenter(policy, crop, 4)
    p = aug.upload(aug.draw(n, hp, wp), "cuda")
    io, lo = aug.apply(image, label, p)
    field = None if p["alpha"] is None else ops.aug_elastic_field(n, hp, wp, p["alpha"], p["sigma"], p["seed"])
    w, l2 = ops.aug_warp(image, label, p["matrix"], p["intensity"], crop, field=field)
    assert torch.equal(io, ops.rescale_intensity(w, 0.0, 1.0)) and torch.equal(lo, l2)
    again = aug.apply(image, label, p)
    assert torch.equal(io, again[0]) and torch.equal(lo, again[1])        # the same bits on every call
    assert tuple(io.shape) == (n, 1) + crop and io.dtype == torch.float32 and tuple(lo.shape) == (n,) + crop and lo.dtype == torch.int64
    flat = io.reshape(n, -1)
    assert torch.all(flat.min(dim=1).values == 0) and torch.all(flat.max(dim=1).values == 1)
    assert set(torch.unique(lo).tolist()) <= set(torch.unique(label).tolist()) | {0}


@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
def test_apply_matches_apply_host(shape):
    (hp, wp), crop = shape
    n = 8
    image, label = _batch(n, hp, wp, 10)
    aug = BatchAugmenter("ACDC_affine_elastic_intensity", crop, 6)
    p = aug.draw(n, hp, wp)
    assert 0 < int(p["elastic_on"].sum()) < n
    pd = aug.upload(p, "cuda")
    io, lo = aug.apply(image, label, pd)
    # the device's own fp32 displacement goes to the oracle, so that both resample at the same place; the field has its own test
    field = ops.aug_elastic_field(n, hp, wp, pd["alpha"], pd["sigma"], pd["seed"]).cpu().numpy()
    host_field = augment.elastic_field_host(p["alpha"].numpy(), p["sigma"].numpy(), hp, wp, seeds=p["seed"].numpy())
    assert np.abs(field - host_field).max() <= 4e-5 * float(p["alpha"].max())
    img_h, lab_h = image.cpu().numpy(), label.cpu().numpy()
    want_i, want_l = augment.apply_host(img_h, lab_h, p, field=field)
    bound, s = warp_bound(img_h, p["matrix"].numpy(), p["intensity"].numpy(), crop, field)
    warped, _ = augment.warp_host(img_h, lab_h, p["matrix"].numpy(), p["intensity"].numpy(), crop, field)
    rng_ = (warped.max(axis=(1, 2, 3)) - warped.min(axis=(1, 2, 3))).reshape(n, 1, 1)
    full = (bound + 3 * bound.max(axis=(1, 2), keepdims=True)) / rng_ + 4 * EPS24
    err = np.abs(io.cpu().numpy()[:, 0].astype(np.float64) - want_i[:, 0])
    print(f"end to end {shape}: max err {err.max():.3e}, max err / bound {np.max(err / full):.3f}")
    assert np.all(err <= full)
    keep = label_mask(s)
    left = 1.0 - keep.reshape(n, -1).mean(axis=1)
    print(f"end to end {shape}: label pixels left out, max {100 * left.max():.3f} %")
    assert np.all(left <= 0.01)
    assert np.array_equal(lo.cpu().numpy()[keep], want_l[keep])


@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_apply_matches_the_pure_host_path(shape):
    """Hash noise -> field -> warp -> rescale on the device against apply_host alone (nothing of the device goes into the oracle).  The
    two displacements differ by up to 4e-5 * alpha px per axis (the field bound), which M carries into the source coordinate: the
    coordinate tolerance of sample b is delta_b = 1e-3 + 4e-5 * alpha_b * max row sum of |M_b|'s 2x2 part, used in the image bound and
    in the band around the label rounding boundaries (about 0.02 px, so a few per cent of the pixels are left out and no cap is set)."""
    (hp, wp), crop = shape
    n = 8
    image, label = _batch(n, hp, wp, 17)
    aug = BatchAugmenter("ACDC_affine_elastic_intensity", crop, 9)
    p = aug.draw(n, hp, wp)
    assert 0 < int(p["elastic_on"].sum()) < n
    io, lo = aug.apply(image, label, aug.upload(p, "cuda"))
    img_h, lab_h = image.cpu().numpy(), label.cpu().numpy()
    want_i, want_l = augment.apply_host(img_h, lab_h, p)
    m, alpha = p["matrix"].numpy().astype(np.float64), p["alpha"].numpy().astype(np.float64)
    delta = DELTA + 4e-5 * alpha * np.abs(m[:, :, :2]).sum(axis=2).max(axis=1)
    field = augment.elastic_field_host(p["alpha"].numpy(), p["sigma"].numpy(), hp, wp, seeds=p["seed"].numpy())
    bound, s = warp_bound(img_h, p["matrix"].numpy(), p["intensity"].numpy(), crop, field, delta=delta)
    warped, _ = augment.warp_host(img_h, lab_h, p["matrix"].numpy(), p["intensity"].numpy(), crop, field)
    rng_ = (warped.max(axis=(1, 2, 3)) - warped.min(axis=(1, 2, 3))).reshape(n, 1, 1)
    full = (bound + 3 * bound.max(axis=(1, 2), keepdims=True)) / rng_ + 4 * EPS24
    err = np.abs(io.cpu().numpy()[:, 0].astype(np.float64) - want_i[:, 0])
    print(f"pure host {shape}: delta max {delta.max():.4f} px, max err {err.max():.3e}, max err / bound {np.max(err / full):.3f}")
    assert np.all(err <= full)
    keep = label_mask(s, delta)
    print(f"pure host {shape}: label pixels left out, max {100 * (1 - keep.reshape(n, -1).mean(axis=1)).max():.2f} %")
    assert keep.mean() > 0.8
    assert np.array_equal(lo.cpu().numpy()[keep], want_l[keep])


def test_constant_plane_follows_rescale_intensity():
    image = torch.full((2, 1, 64, 64), 3.0, device="cuda")
    label = dev(blobs(2, 64, 64, 11))
    aug = BatchAugmenter("no_aug", (48, 48), 0)
    io, _ = aug.apply(image, label, aug.upload(aug.draw(2, 64, 64), "cuda"))
    assert torch.equal(io, ops.rescale_intensity(image[:, :, 8:56, 8:56].contiguous()))
    assert torch.count_nonzero(io) == 0


def test_call_out_and_stream():
    n, hp, wp, crop = 4, 224, 224, (192, 192)
    image, label = _batch(n, hp, wp, 12)
    aug = BatchAugmenter("ACDC_affine_elastic_intensity", crop, 2)
    p = aug.upload(aug.draw(n, hp, wp), "cuda")
    want = aug.apply(image, label, p)
    io, lo = torch.empty((n, 1) + crop, device="cuda"), torch.empty((n,) + crop, dtype=torch.int64, device="cuda")
    got = aug.apply(image, label, p, out=(io, lo))
    assert got[0] is io and got[1] is lo and torch.equal(io, want[0]) and torch.equal(lo, want[1])
    with pytest.raises(_ffi.CtlError, match="overlaps"):
        aug.apply(image, label, p, out=(io, label.view(-1)[:n * 192 * 192].view((n,) + crop)))      # a view into the input label
    with pytest.raises(ValueError, match="shares memory"):
        aug.apply(image, label, p, out=(image.view(-1)[:n * 192 * 192].view((n, 1) + crop), lo))    # a view into the input image
    assert torch.equal(io, want[0]) and torch.equal(lo, want[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = aug.apply(image, label, p)
    side.synchronize()
    assert torch.equal(on_side[0], want[0]) and torch.equal(on_side[1], want[1])
    a, b = BatchAugmenter("ACDC_affine_elastic_intensity", crop, 21), BatchAugmenter("ACDC_affine_elastic_intensity", crop, 21)
    ra, rb = a(image, label), b(image, label)                   # draw + upload + apply; the same seed gives the same batch
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    rc = a(image, label)
    assert not torch.equal(ra[0], rc[0])
    hi, hl = aug.apply(image.cpu().numpy(), label.cpu().numpy(), aug.draw(n, hp, wp))       # numpy inputs: the host path
    assert isinstance(hi, np.ndarray) and hi.shape == (n, 1) + crop and hl.shape == (n,) + crop


def test_graph_replay_equals_eager():
    n, hp, wp, crop = 8, 224, 224, (192, 192)
    aug = BatchAugmenter("ACDC_affine_elastic_intensity", crop, 3)
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
    hp, wp, crop = 224, 224, (192, 192)
    image, label = _batch(n, hp, wp, 16)
    for policy, launches in (("ACDC_affine_elastic_intensity", 6), ("ACDC_affine_intensity", 4)):
        aug = BatchAugmenter(policy, crop, 1)
        p = aug.upload(aug.draw(n, hp, wp), "cuda")
        before = _ffi.lib.ctl_launch_count()
        aug.apply(image, label, p)
        assert _ffi.lib.ctl_launch_count() - before == launches, (policy, n)
