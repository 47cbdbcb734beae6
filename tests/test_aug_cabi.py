"""Batch augmentation without a GPU: the C-ABI boundary of ctl_aug_ws_bytes / ctl_aug_field / ctl_aug_warp (declared, exported, bound,
every argument error refused before a launch), the policy table, the parameter draw, the composed matrices, and the host statement of
the semantics (augment.apply_host) on the cases whose result can be written down by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, augment
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ctl_aug_ws_bytes", "ctl_aug_warp_ws_bytes", "ctl_aug_field", "ctl_aug_warp")


def _header():
    return open(os.path.join(ROOT, "include", "ctl_hip.h")).read()


def test_entries_declared_exported_bound():
    header = _header()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _ffi.EXPORTED
        assert getattr(_ffi.lib, name).argtypes is not None
    assert _ffi.lib.ctl_aug_ws_bytes.restype is C.c_size_t and _ffi.lib.ctl_aug_warp_ws_bytes.restype is C.c_size_t
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == _ffi.ABI_VERSION == _ffi.lib.ctl_version()


def test_header_cites_the_reference_lines():
    header = _header()
    section = header[header.index("training augmentation"):header.index("size_t ctl_aug_ws_bytes")]
    for cite in ("transform.py:46-86", "affine_transform.py:280-283", "intensity_transform.py:136-162", "elastic_transform.py:41-58",
                 "transform.py:83-84", "affine_transform.py:200-244", "affine_transform.py:750-804"):
        assert cite in section, cite


def test_ws_bytes():
    field_ws, ws = _ffi.lib.ctl_aug_ws_bytes, _ffi.lib.ctl_aug_warp_ws_bytes
    assert field_ws(1, 37, 53) > 0 and field_ws(16, 224, 224) >= 16 * 2 * 224 * 224 * 4 and field_ws(16, 512, 512) > 0
    sizes = [field_ws(n, s, s) for n, s in ((1, 64), (1, 128), (2, 128), (16, 256), (16, 512), (32, 512))]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    for bad in ((16, 513, 256), (16, 256, 513), (0, 256, 256), (-1, 256, 256), (16, 0, 256), (16, 256, -4), (70000, 64, 64)):
        assert field_ws(*bad) == 0, bad
    assert ws(1, 37, 53, 20, 20) > 0 and ws(16, 512, 512, 512, 512) > 0
    assert 16 * 64 * 2 * 4 <= ws(16, 224, 224, 192, 192) < 16 * 224 * 224          # the partials, not a plane
    sizes = [ws(n, 64, 64, 64, 64) for n in (1, 2, 16, 64, 1024)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    for bad in ((16, 513, 256, 192, 192), (16, 256, 513, 192, 192), (0, 256, 256, 192, 192), (-1, 256, 256, 192, 192),
                (16, 0, 256, 1, 1), (16, 256, -4, 1, 1), (16, 256, 256, 0, 192), (16, 256, 256, 192, -1),
                (16, 224, 224, 225, 192), (16, 224, 224, 192, 225)):
        assert ws(*bad) == 0, bad


FAKE = 0x10000        # a non-null, 256-byte aligned address that is never dereferenced: every case below is refused before a launch


def _field_args(**kw):
    a = dict(noise=None, seeds=FAKE * 8, alpha=FAKE * 9, sigma=FAKE * 10, n=2, hp=64, wp=64, field=FAKE, ws=FAKE * 4, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return [a[k] for k in ("noise", "seeds", "alpha", "sigma", "n", "hp", "wp", "field", "ws", "ws_bytes", "stream")]


def _warp_args(**kw):
    a = dict(image=FAKE, label=FAKE * 2, matrix=FAKE * 8, intensity=FAKE * 9, field=None, n=2, hp=64, wp=64, hc=48, wc=48, image_out=FAKE * 3,
             label_out=FAKE * 4, ws=FAKE * 10, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return [a[k] for k in ("image", "label", "matrix", "intensity", "field", "n", "hp", "wp", "hc", "wc", "image_out", "label_out", "ws",
                           "ws_bytes", "stream")]


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "positive"), (dict(hp=-1), "positive"), (dict(wp=0), "positive"), (dict(n=70000), "65535"),
    (dict(hp=513), "512"), (dict(wp=600), "512"), (dict(seeds=None), "seeds"), (dict(alpha=None), "alpha"), (dict(sigma=None), "sigma"),
    (dict(field=None), "field"), (dict(ws=None), "workspace"), (dict(ws=FAKE + 4), "aligned"), (dict(ws_bytes=1024), "ctl_aug_ws_bytes"),
    (dict(noise=FAKE * 5, field=FAKE * 5), "overlap"), (dict(noise=FAKE * 5, field=FAKE * 5 + 256), "overlap"),
    (dict(ws=FAKE * 16, field=FAKE * 16 + 1024), "overlap"), (dict(alpha=FAKE * 7, field=FAKE * 7), "overlap")])
def test_field_argument_errors(kw, word):
    before = _ffi.lib.ctl_launch_count()
    assert _ffi.lib.ctl_aug_field(*_field_args(**kw)) == -1
    msg = _ffi.lib.ctl_last_error().decode()
    assert msg.startswith("aug_field:") and word in msg, msg
    assert _ffi.lib.ctl_launch_count() == before
    with pytest.raises(_ffi.CtlError, match="aug_field"):
        _ffi.check(-1, "ctl_aug_field")


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "positive"), (dict(hc=0), "positive"), (dict(wc=-3), "positive"), (dict(hp=0), "positive"), (dict(hp=513, hc=48), "512"),
    (dict(wp=1024), "512"), (dict(hc=65), "larger"), (dict(wc=65), "larger"), (dict(image=None), "image"), (dict(label=None), "label"),
    (dict(matrix=None), "matrix"), (dict(intensity=None), "intensity"), (dict(image_out=None), "image_out"),
    (dict(label_out=None), "label_out"), (dict(ws=None), "workspace"), (dict(ws=FAKE + 8), "aligned"), (dict(ws_bytes=0), "ctl_aug_warp_ws_bytes"),
    (dict(image_out=FAKE + 64), "overlaps"), (dict(label_out=FAKE * 2), "overlaps"), (dict(label_out=FAKE * 3 + 512), "overlaps"),
    (dict(field=FAKE * 3), "overlaps"), (dict(ws=FAKE * 4), "overlaps"), (dict(matrix=FAKE * 3), "overlaps")])
def test_warp_argument_errors(kw, word):
    before = _ffi.lib.ctl_launch_count()
    assert _ffi.lib.ctl_aug_warp(*_warp_args(**kw)) == -1
    msg = _ffi.lib.ctl_last_error().decode()
    assert msg.startswith("aug_warp:") and word in msg, msg
    assert _ffi.lib.ctl_launch_count() == before


# ---------------------------------------------------------------------------------------------- policies and the draw
ACDC = dict(flip=(True, True, 0.2), shift=(0.1, 0.1), rotate=15.0, scale=(0.8, 1.1), shear=0.0,
            rotate_groups=(0, 45, 90, 135, 180, 225, 270, 315))
PLAIN = dict(flip=(False, False, 0.0), shift=(0.0, 0.0), rotate=0.0, scale=(1.0, 1.0), shear=0.0, rotate_groups=())
AFFINE = dict(PLAIN, shift=(0.1, 0.1), rotate=15.0, scale=(0.9, 1.1))
TABLE = {       # transform.py:114-313
    "no_aug": dict(PLAIN, intensity_prob=0.0, elastic_prob=0.0),
    "affine": dict(AFFINE, intensity_prob=0.0, elastic_prob=0.0),
    "scale": dict(PLAIN, scale=(0.8, 1.2), intensity_prob=0.0, elastic_prob=0.0),
    "elastic": dict(PLAIN, intensity_prob=0.0, elastic_prob=1.0),
    "elastic_scale": dict(PLAIN, scale=(0.9, 1.1), intensity_prob=0.0, elastic_prob=0.5),
    "affine_elastic": dict(AFFINE, intensity_prob=0.0, elastic_prob=0.5),
    "ACDC_affine": dict(ACDC, intensity_prob=0.0, elastic_prob=0.0),
    "ACDC_affine_intensity": dict(ACDC, intensity_prob=0.5, elastic_prob=0.0),
    "ACDC_affine_elastic": dict(ACDC, intensity_prob=0.0, elastic_prob=0.5),
    "ACDC_affine_elastic_intensity": dict(ACDC, intensity_prob=0.5, elastic_prob=0.5),
    "Prostate_affine_elastic_intensity": dict(PLAIN, flip=(True, True, 0.5), shift=(0.1, 0.1), rotate=15.0, scale=(0.8, 1.2),
                                              intensity_prob=0.5, elastic_prob=0.5),
}


def test_policy_table():
    assert set(augment.POLICIES) == set(TABLE)
    for name, want in TABLE.items():
        assert augment.POLICIES[name] == want, name
    assert augment.CONTRAST_RANGE == (0.8, 1.2) and augment.BRIGHTNESS_RANGE == (-0.1, 0.1)
    assert augment.ALPHA_RANGE == (1.5, 2.0) and augment.SIGMA_RANGE == (0.1, 0.2) and augment.SIGMA_FACTOR == 0.75


@pytest.mark.parametrize("name, needs", [
    ("gamma", "RandomGamma"), ("Atrial_basic", "RandomGamma"), ("affine_gamma_elastic", "RandomGamma"),
    ("ACDC_affine_perturb", "MyRandomPurtarbation"), ("ACDC_affine_perturb_v2", "MyRandomPurtarbationV2"),
    ("ACDC_affine_all", "MyRandomPurtarbationV2"), ("ACDC_affine_elastic_bias", "MyRandomPurtarbationV2"),
    ("ACDC_affine_elastic_intensity_v2", "MyElasticTransformCoarseGrid"), ("elastic_v2", "MyElasticTransformCoarseGrid")])
def test_unsupported_policy_names_the_transform(name, needs):
    with pytest.raises(NotImplementedError, match=needs):
        BatchAugmenter(name, (192, 192), 0)


REFERENCE_NAMES = {       # every key of aug_config, transform.py:16-41
    "no_aug", "gamma", "gamma_scale", "affine", "scale", "elastic", "elastic_scale", "gamma_elastic", "affine_elastic", "affine_gamma",
    "affine_gamma_elastic", "ACDC_affine", "ACDC_affine_perturb", "ACDC_affine_perturb_v2", "ACDC_affine_elastic", "ACDC_affine_intensity",
    "ACDC_affine_elastic_intensity", "ACDC_affine_elastic_intensity_v2", "ACDC_affine_elastic_bias", "ACDC_affine_all", "Atrial_basic",
    "Atrial_perturb", "Prostate_affine_elastic_intensity", "elastic_v2"}


def test_every_reference_name_is_supported_or_refused_by_name():
    assert set(augment.POLICIES) | set(augment.UNSUPPORTED) == REFERENCE_NAMES
    assert not set(augment.POLICIES) & set(augment.UNSUPPORTED)
    for name in augment.UNSUPPORTED:
        with pytest.raises(NotImplementedError):
            augment.get_policy(name)


def test_unknown_policy():
    with pytest.raises(KeyError):
        BatchAugmenter("nope", (192, 192), 0)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


def test_draw_is_deterministic_per_seed():
    a = BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 7).draw(16, 224, 224)
    b = BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 7).draw(16, 224, 224)
    c = BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 8).draw(16, 224, 224)
    _same(a, b)
    assert not torch.equal(a["matrix"], c["matrix"]) and not torch.equal(a["seed"], c["seed"])
    assert a["matrix"].dtype == torch.float32 and tuple(a["matrix"].shape) == (16, 2, 3)
    assert a["intensity"].dtype == torch.float32 and tuple(a["intensity"].shape) == (16, 2)
    assert a["alpha"].dtype == a["sigma"].dtype == torch.float32 and a["seed"].dtype == torch.int64
    assert a["crop"].tolist() == [192, 192] and not any(v.is_cuda for v in a.values())
    none = BatchAugmenter("ACDC_affine_intensity", (192, 192), 7).draw(4, 224, 224)
    assert none["alpha"] is None and none["sigma"] is None and none["seed"] is None


def _within_3_sd(hits, n, p):
    assert abs(int(hits) - n * p) <= 3.0 * np.sqrt(n * p * (1 - p)), (int(hits), n, p)


def test_draw_ranges_and_probabilities():
    n, hp, wp = 10000, 224, 208
    d = BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 3).draw(n, hp, wp)
    g = {k: (None if v is None else v.numpy()) for k, v in d.items()}
    _within_3_sd(g["flip"][:, 0].sum(), n, 0.2)
    _within_3_sd(g["flip"][:, 1].sum(), n, 0.2)
    _within_3_sd(g["intensity_on"].sum(), n, 0.5)
    _within_3_sd(g["elastic_on"].sum(), n, 0.5)
    _within_3_sd((g["flip"][:, 0] & g["flip"][:, 1]).sum(), n, 0.04)          # the two flips are independent
    assert np.all(np.abs(g["theta"]) <= 15) and g["theta"].min() < -14 and g["theta"].max() > 14
    assert np.all(np.abs(g["translate"]) <= 0.1) and g["translate"].min() < -0.09 and g["translate"].max() > 0.09
    assert np.all((g["zoom"] >= 0.8) & (g["zoom"] <= 1.1)) and g["zoom"].min() < 0.81 and g["zoom"].max() > 1.09
    assert np.abs(g["zoom"][:, 0] - g["zoom"][:, 1]).max() > 0.2            # independent zooms per axis
    assert set(np.unique(g["choice"])) == {0, 45, 90, 135, 180, 225, 270, 315}
    for a in range(8):
        _within_3_sd((g["choice"] == 45 * a).sum(), n, 1 / 8)
    on = g["intensity_on"]
    assert np.all(g["contrast"][~on] == 1) and np.all(g["brightness"][~on] == 0)
    assert np.all((g["contrast"][on] >= 0.8) & (g["contrast"][on] <= 1.2)) and np.all(np.abs(g["brightness"][on]) <= 0.1)
    assert np.array_equal(g["intensity"], np.stack([g["contrast"], g["brightness"]], 1).astype(np.float32))
    el = g["elastic_on"]
    assert np.all(g["alpha"][~el] == 0)
    assert np.all((g["alpha"][el] >= np.float32(1.5 * hp)) & (g["alpha"][el] <= np.float32(2.0 * hp)))
    assert np.all((g["sigma"] >= np.float32(0.075 * hp)) & (g["sigma"] <= np.float32(0.15 * hp)))
    assert len(np.unique(g["seed"])) == n and g["seed"].min() >= 0
    assert np.array_equal(g["matrix"], augment.compose_matrix(g["flip"], g["theta"], g["translate"], g["zoom"], g["choice"], hp, wp).astype(np.float32))
    p = BatchAugmenter("Prostate_affine_elastic_intensity", (192, 192), 3).draw(n, hp, wp)
    _within_3_sd(p["flip"][:, 0].sum(), n, 0.5)
    assert np.all(p["choice"].numpy() == 0)
    e = BatchAugmenter("elastic", (192, 192), 3).draw(100, hp, wp)
    assert bool(e["elastic_on"].all()) and np.array_equal(e["matrix"].numpy(), np.tile(np.float32([[1, 0, 0], [0, 1, 0]]), (100, 1, 1)))


def _m(flip=(False, False), theta=0.0, translate=(0.0, 0.0), zoom=(1.0, 1.0), choice=0.0, hp=64, wp=48):
    return augment.compose_matrix([flip], [theta], [translate], [zoom], [choice], hp, wp)[0]


def test_composed_matrices_by_hand():
    assert np.array_equal(_m(), [[1, 0, 0], [0, 1, 0]])
    assert np.array_equal(_m(flip=(True, False)), [[1, 0, 0], [0, -1, 0]])          # horizontal: columns reversed
    assert np.array_equal(_m(flip=(False, True)), [[-1, 0, 0], [0, 1, 0]])          # vertical: rows reversed
    assert np.array_equal(_m(flip=(True, True)), [[-1, 0, 0], [0, -1, 0]])
    assert np.array_equal(_m(choice=90.0), [[0, -1, 0], [1, 0, 0]])
    assert np.array_equal(_m(theta=90.0), [[0, -1, 0], [1, 0, 0]])
    assert np.array_equal(_m(choice=180.0), [[-1, 0, 0], [0, -1, 0]])
    assert np.array_equal(_m(choice=270.0), [[0, 1, 0], [-1, 0, 0]])
    assert np.array_equal(_m(translate=(0.125, -0.25)), [[1, 0, 8], [0, 1, -12]])  # fractions of 64 rows / 48 columns
    assert np.array_equal(_m(zoom=(0.5, 2.0)), [[0.5, 0, 0], [0, 2, 0]])
    r = np.sqrt(0.5)
    assert np.allclose(_m(choice=45.0), [[r, -r, 0], [r, r, 0]], atol=1e-15)
    # M = F R(theta) T Z Rc: the translation is rotated by theta and flipped, the zoom sits between T and Rc
    got = _m(flip=(True, False), theta=90.0, translate=(0.125, 0.0), zoom=(2.0, 1.0), choice=90.0)
    f, rot, t, z = np.diag([1.0, -1, 1]), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.eye(3), np.diag([2.0, 1, 1])
    t[0, 2] = 8
    assert np.array_equal(got, (f @ rot @ t @ z @ rot)[:2])


# ---------------------------------------------------------------------------------------------- apply_host
def _batch(n, hp, wp, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((n, 1, hp, wp), dtype=np.float32) * 3 - 1, rng.integers(0, 4, (n, hp, wp), dtype=np.int64)


def _params(n, hp, wp, crop, **kw):
    m = augment.compose_matrix(kw.get("flip", [(False, False)] * n), kw.get("theta", [0.0] * n), kw.get("translate", [(0.0, 0.0)] * n),
                               kw.get("zoom", [(1.0, 1.0)] * n), kw.get("choice", [0.0] * n), hp, wp)
    return {"matrix": torch.from_numpy(m.astype(np.float32)), "intensity": torch.tensor([[1.0, 0.0]] * n), "alpha": kw.get("alpha"),
            "sigma": kw.get("sigma"), "seed": kw.get("seed"), "crop": torch.tensor(crop)}


def _rescale(x):
    x = x.astype(np.float64)
    mn, mx = x.min(axis=(-2, -1), keepdims=True), x.max(axis=(-2, -1), keepdims=True)
    return ((x - mn) / (mx - mn + 1e-20)).astype(np.float32)


def test_apply_host_no_aug_is_centre_crop_and_rescale():
    image, label = _batch(3, 41, 54)
    aug = BatchAugmenter("no_aug", (30, 33), 0)
    io, lo = aug.apply(image, label, aug.draw(3, 41, 54))       # numpy inputs take the host path
    cy, cx = 6, 11                                              # ceil(11 / 2), ceil(21 / 2)
    assert io.dtype == np.float32 and lo.dtype == np.int64
    assert np.array_equal(lo, label[:, cy:cy + 30, cx:cx + 33])
    assert np.array_equal(io, _rescale(image[:, :, cy:cy + 30, cx:cx + 33]))
    assert io.min() == 0 and np.all(io.max(axis=(1, 2, 3)) == 1)


def test_apply_host_flips_equal_np_flip():
    image, label = _batch(3, 40, 56, 1)
    p = _params(3, 40, 56, (40, 56), flip=[(True, False), (False, True), (True, True)])
    io, lo = augment.apply_host(image, label, p)
    for b, axes in enumerate([(-1,), (-2,), (-2, -1)]):
        assert np.array_equal(lo[b], np.flip(label[b], axes))
        assert np.array_equal(io[b], _rescale(np.flip(image[b], axes)))


def test_apply_host_quarter_turns_equal_np_rot90():
    image, label = _batch(3, 48, 48, 2)
    io, lo = augment.apply_host(image, label, _params(3, 48, 48, (48, 48), choice=[90.0, 180.0, 270.0]))
    for b, k in enumerate((-1, 2, 1)):        # out[i, j] = in[N - 1 - j, i] for 90 degrees: np.rot90 with k = -1
        assert np.array_equal(lo[b], np.rot90(label[b], k))
        assert np.array_equal(io[b, 0], _rescale(np.rot90(image[b, 0], k)))


def test_apply_host_zero_alpha_elastic_changes_nothing():
    image, label = _batch(2, 40, 40, 3)
    plain = augment.apply_host(image, label, _params(2, 40, 40, (32, 32), theta=[10.0, -5.0]))
    zero = augment.apply_host(image, label, _params(2, 40, 40, (32, 32), theta=[10.0, -5.0], alpha=torch.zeros(2),
                                                    sigma=torch.tensor([4.0, 6.0]), seed=torch.tensor([1, 2])))
    assert np.array_equal(plain[0], zero[0]) and np.array_equal(plain[1], zero[1])
    live = augment.apply_host(image, label, _params(2, 40, 40, (32, 32), theta=[10.0, -5.0], alpha=torch.tensor([60.0, 0.0]),
                                                    sigma=torch.tensor([4.0, 6.0]), seed=torch.tensor([1, 2])))
    assert not np.array_equal(plain[0][0], live[0][0]) and np.array_equal(plain[0][1], live[0][1])


def test_hash_noise_is_uniform_and_keyed():
    u = augment.hash_noise([5, 5, 6], 64, 64)
    assert u.min() >= -1 and u.max() < 1
    n = u[0].size
    assert abs(u[0].mean()) < 5 * np.sqrt(1 / 3 / n) and abs(u[0].var() - 1 / 3) < 5 * np.sqrt(4 / 45 / n)
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u[0, 0], u[0, 1]) and not np.array_equal(u[1], u[2])
    assert np.array_equal(u[:2], augment.hash_noise([5, 5], 64, 64))
