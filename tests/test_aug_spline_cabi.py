"""Cubic-spline resampling of the batch augmenter without a GPU: the C-ABI boundary of ctl_aug_spline_ws_bytes / ctl_aug_warp_cubic_ws_bytes /
ctl_aug_spline_coeffs / ctl_aug_warp_cubic (declared, exported, bound, every argument error refused before a launch) and the host
statement of the semantics (augment.warp_host(interp="cubic")) against scipy called directly."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, augment
from cooperative_training_and_latent_space_data_augmentation_amd.augment import BatchAugmenter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ctl_aug_spline_ws_bytes", "ctl_aug_warp_cubic_ws_bytes", "ctl_aug_spline_coeffs", "ctl_aug_warp_cubic")


def test_entries_declared_exported_bound():
    header = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _ffi.EXPORTED
        assert getattr(_ffi.lib, name).argtypes is not None
    assert _ffi.lib.ctl_aug_spline_ws_bytes.restype is C.c_size_t and _ffi.lib.ctl_aug_warp_cubic_ws_bytes.restype is C.c_size_t
    assert int(re.search(r"#define\s+CTL_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == _ffi.ABI_VERSION == _ffi.lib.ctl_version()
    # ctl_aug_warp keeps its signature
    assert re.search(r"int ctl_aug_warp\(const float\* image, const int64_t\* label, const float\* matrix, const float\* intensity, "
                     r"const float\* field, int32_t n,\s+int32_t hp, int32_t wp, int32_t hc, int32_t wc, float\* image_out, int64_t\* label_out, "
                     r"void\* workspace,\s+size_t workspace_bytes, ctl_stream stream\);", header)
    assert len(_ffi.lib.ctl_aug_warp.argtypes) == 15 and len(_ffi.lib.ctl_aug_warp_cubic.argtypes) == 16


def test_ws_bytes():
    coeffs_ws, warp_ws = _ffi.lib.ctl_aug_spline_ws_bytes, _ffi.lib.ctl_aug_warp_cubic_ws_bytes
    plane = 224 * 224 * 4
    assert coeffs_ws(16, 224, 224, 4) >= 16 * 5 * plane and warp_ws(16, 224, 224, 192, 192, 4) >= 2 * 16 * 5 * plane
    assert warp_ws(16, 224, 224, 192, 192, 4) > coeffs_ws(16, 224, 224, 4) > coeffs_ws(16, 224, 224, 0) > 0
    assert coeffs_ws(1, 5, 7, 0) > 0 and warp_ws(1, 5, 7, 5, 7, 1) > 0 and warp_ws(32, 512, 512, 512, 512, 16) > 0
    sizes = [warp_ws(n, 64, 64, 64, 64, k) for n, k in ((1, 1), (1, 2), (2, 2), (16, 4), (16, 16))]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    for bad in ((16, 513, 256, 4), (16, 256, 513, 4), (0, 256, 256, 4), (-1, 256, 256, 4), (16, 0, 256, 4), (70000, 64, 64, 4),
                (16, 256, 256, 17), (16, 256, 256, -1)):
        assert coeffs_ws(*bad) == 0, bad
    for bad in ((16, 513, 256, 192, 192, 4), (16, 256, 513, 192, 192, 4), (0, 256, 256, 192, 192, 4), (16, 256, 256, 0, 192, 4),
                (16, 256, 256, 192, -1, 4), (16, 224, 224, 225, 192, 4), (16, 224, 224, 192, 225, 4), (16, 224, 224, 192, 192, 17),
                (16, 224, 224, 192, 192, 0), (70000, 64, 64, 64, 64, 4)):
        assert warp_ws(*bad) == 0, bad


FAKE = 0x10000000     # non-null, 256-byte aligned, never dereferenced: every case below is refused before a launch


def _coeffs_args(**kw):
    a = dict(image=FAKE, label=FAKE * 2, intensity=FAKE * 3, n=2, hp=64, wp=64, n_class=4, coeffs=FAKE * 4, ws=FAKE * 5, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return [a[k] for k in ("image", "label", "intensity", "n", "hp", "wp", "n_class", "coeffs", "ws", "ws_bytes", "stream")]


def _warp_args(**kw):
    a = dict(image=FAKE, label=FAKE * 2, matrix=FAKE * 8, intensity=FAKE * 9, field=None, n=2, hp=64, wp=64, hc=48, wc=48, n_class=4,
             image_out=FAKE * 3, label_out=FAKE * 4, ws=FAKE * 10, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return [a[k] for k in ("image", "label", "matrix", "intensity", "field", "n", "hp", "wp", "hc", "wc", "n_class", "image_out", "label_out",
                           "ws", "ws_bytes", "stream")]


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "positive"), (dict(hp=-1), "positive"), (dict(wp=0), "positive"), (dict(n=70000), "65535"), (dict(hp=513), "512"),
    (dict(wp=600), "512"), (dict(n_class=17), "n_class"), (dict(n_class=-1), "n_class"), (dict(image=None), "image"),
    (dict(intensity=None), "intensity"), (dict(label=None), "label"), (dict(coeffs=None), "coeffs"), (dict(ws=None), "workspace"),
    (dict(ws=FAKE * 5 + 4), "aligned"), (dict(ws_bytes=4096), "ctl_aug_spline_ws_bytes"), (dict(coeffs=FAKE), "overlap"),
    (dict(coeffs=FAKE * 2 + 64), "overlap"), (dict(coeffs=FAKE * 5 + 1024), "overlap"), (dict(ws=FAKE * 3), "overlap")])
def test_coeffs_argument_errors(kw, word):
    before = _ffi.lib.ctl_launch_count()
    assert _ffi.lib.ctl_aug_spline_coeffs(*_coeffs_args(**kw)) == -1
    msg = _ffi.lib.ctl_last_error().decode()
    assert msg.startswith("aug_spline_coeffs:") and word in msg, msg
    assert _ffi.lib.ctl_launch_count() == before


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "positive"), (dict(hc=0), "positive"), (dict(wc=-3), "positive"), (dict(hp=0), "positive"), (dict(hp=513, hc=48), "512"),
    (dict(wp=1024), "512"), (dict(hc=65), "larger"), (dict(wc=65), "larger"), (dict(n_class=17), "n_class"), (dict(n_class=0), "n_class"),
    (dict(image=None), "image"), (dict(label=None), "label"), (dict(matrix=None), "matrix"), (dict(intensity=None), "intensity"),
    (dict(image_out=None), "image_out"), (dict(label_out=None), "label_out"), (dict(ws=None), "workspace"), (dict(ws=FAKE * 10 + 8), "aligned"),
    (dict(ws_bytes=2 * 64 * 2 * 4), "ctl_aug_warp_cubic_ws_bytes"), (dict(ws_bytes=_ffi.lib.ctl_aug_spline_ws_bytes(2, 64, 64, 4)), "ctl_aug_warp_cubic_ws_bytes"),
    (dict(image_out=FAKE + 64), "overlaps"), (dict(label_out=FAKE * 2), "overlaps"), (dict(label_out=FAKE * 3 + 512), "overlaps"),
    (dict(field=FAKE * 3), "overlaps"), (dict(ws=FAKE * 4), "overlaps"), (dict(matrix=FAKE * 3), "overlaps"), (dict(image=FAKE * 10 + 4096), "overlaps")])
def test_warp_cubic_argument_errors(kw, word):
    before = _ffi.lib.ctl_launch_count()
    assert _ffi.lib.ctl_aug_warp_cubic(*_warp_args(**kw)) == -1
    msg = _ffi.lib.ctl_last_error().decode()
    assert msg.startswith("aug_warp_cubic:") and word in msg, msg
    assert _ffi.lib.ctl_launch_count() == before
    with pytest.raises(_ffi.CtlError, match="aug_warp_cubic"):
        _ffi.check(-1, "ctl_aug_warp_cubic")


# ---------------------------------------------------------------------------------------------- warp_host(interp="cubic")
def _case(n=2, hp=23, wp=31, crop=(20, 27), seed=0):
    rng = np.random.default_rng(seed)
    image = (rng.random((n, 1, hp, wp), dtype=np.float32) * 3 - 1)
    label = rng.integers(0, 4, (n, hp, wp), dtype=np.int64)
    label[:, 5:15, 8:20] = 3
    label[:, 9:12, 10:16] = 1
    matrix = augment.compose_matrix([(False, True), (True, False)][:n], [12.0, -7.0][:n], [(0.1, -0.05), (0.0, 0.08)][:n], [(0.9, 1.1), (1.3, 1.25)][:n],
                                    [45.0, 0.0][:n], hp, wp).astype(np.float32)
    intensity = np.float32([[1.2, 0.1], [0.8, -0.1]])[:n]
    field = (rng.random((n, 2, hp, wp)) * 2 - 1).astype(np.float32)
    return image, label, matrix, intensity, crop, field


def test_warp_host_cubic_is_map_coordinates_inside_and_zero_outside():
    image, label, matrix, intensity, crop, field = _case()
    n, _, hp, wp = image.shape
    io, lo = augment.warp_host(image, label, matrix, intensity, crop, field, interp="cubic", n_class=4)
    s = augment.source_coords(matrix, hp, wp, crop[0], crop[1], field)
    seen = set()
    for b in range(n):
        inside = (s[b, 0] >= -0.5) & (s[b, 0] <= hp - 0.5) & (s[b, 1] >= -0.5) & (s[b, 1] <= wp - 0.5)
        assert 0 < inside.sum() < inside.size
        x = image[b, 0].astype(np.float64)
        v = np.clip(x * float(intensity[b, 0]) + float(intensity[b, 1]), x.min(), x.max())
        want = ndimage.map_coordinates(v, s[b], order=3, mode="reflect")
        assert np.array_equal(io[b, 0][inside], want[inside])
        assert np.all(io[b, 0][~inside] == 0) and np.all(lo[b][~inside] == 0)
        assert np.count_nonzero(want[~inside]) > 0                    # scipy alone would have reflected the border into view
        # the largest k whose indicator value is >= 0.5, 0 if there is none
        vals = np.stack([ndimage.map_coordinates((label[b] == k).astype(np.float64), s[b], order=3, mode="reflect") for k in range(4)])
        for i, j in zip(*np.nonzero(inside)):
            over = [k for k in range(4) if vals[k, i, j] >= 0.5]
            assert lo[b, i, j] == (max(over) if over else 0)
            seen.add((len(over), lo[b, i, j]))
    assert {n_over for n_over, _ in seen} >= {0, 1}                   # pixels with no class at 0.5 exist, and take label 0
    assert io.dtype == np.float64 and lo.dtype == np.int64 and io.shape == (n, 1) + crop and lo.shape == (n,) + crop


def test_warp_host_cubic_largest_class_wins_and_foreign_labels_vanish():
    hp = wp = 12
    label = np.zeros((1, hp, wp), dtype=np.int64)
    label[0, :, 6:] = 2
    image = np.zeros((1, 1, hp, wp), dtype=np.float32)
    matrix, intensity = np.float32([[[1, 0, 0], [0, 1, 0.5]]]), np.float32([[1, 0]])          # half a pixel along the columns
    _, lo = augment.warp_host(image, label, matrix, intensity, (hp, wp), interp="cubic", n_class=3)
    # midway between class 0 and class 2 both indicators are exactly 0.5 up to rounding; away from the edge the classes are plain
    assert np.all(lo[0, :, :5] == 0) and np.all(lo[0, :, 6:11] == 2) and set(np.unique(lo)) <= {0, 2}
    _, lo2 = augment.warp_host(image, label, matrix, intensity, (hp, wp), interp="cubic", n_class=2)
    assert np.all(lo2 == 0)                                           # label 2 is outside [0, 2): it belongs to no class
    ident = np.float32([[[1, 0, 0], [0, 1, 0]]])
    _, lo3 = augment.warp_host(image, label, ident, intensity, (hp, wp), interp="cubic", n_class=3)
    assert np.array_equal(lo3, label)
    with pytest.raises(ValueError, match="n_class"):
        augment.warp_host(image, label, ident, intensity, (hp, wp), interp="cubic")
    with pytest.raises(ValueError, match="interp"):
        augment.warp_host(image, label, ident, intensity, (hp, wp), interp="nearest")


def test_warp_host_linear_is_unchanged_by_the_new_arguments():
    image, label, matrix, intensity, crop, field = _case(seed=1)
    a = augment.warp_host(image, label, matrix, intensity, crop, field)
    b = augment.warp_host(image, label, matrix, intensity, crop, field, interp="linear", n_class=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = augment.warp_host(image, label, matrix, intensity, crop, field, interp="cubic", n_class=4)
    assert not np.array_equal(a[0], c[0])


def test_apply_host_cubic_is_warp_host_and_rescale():
    image, label, matrix, intensity, crop, field = _case(seed=2)
    params = {"matrix": torch.from_numpy(matrix), "intensity": torch.from_numpy(intensity), "alpha": None, "sigma": None, "seed": None,
              "crop": torch.tensor(crop)}
    io, lo = augment.apply_host(image, label, params, field=field, interp="cubic", n_class=4)
    wi, wl = augment.warp_host(image, label, matrix, intensity, crop, field, interp="cubic", n_class=4)
    assert np.array_equal(io, augment.rescale_host(wi).astype(np.float32)) and np.array_equal(lo, wl)
    aug = BatchAugmenter("no_aug", crop, 0, interp="cubic", num_classes=4)
    hi, hl = aug.apply(image, label, params)                          # numpy inputs: the host path, with the augmenter's interpolation
    want = augment.apply_host(image, label, params, interp="cubic", n_class=4)
    assert np.array_equal(hi, want[0]) and np.array_equal(hl, want[1])


# ---------------------------------------------------------------------------------------------- the augmenter
def test_cubic_needs_num_classes():
    with pytest.raises(ValueError, match="num_classes"):
        BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 0, interp="cubic")
    with pytest.raises(ValueError, match="num_classes"):
        BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 0, interp="cubic", num_classes=17)
    with pytest.raises(ValueError, match="interp"):
        BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 0, interp="spline")
    aug = BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 0, interp="cubic", num_classes=4)
    assert aug.interp == "cubic" and aug.num_classes == 4
    assert BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 0).interp == "linear"


def test_draw_does_not_depend_on_interp():
    a = BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 7)
    b = BatchAugmenter("ACDC_affine_elastic_intensity", (192, 192), 7, interp="cubic", num_classes=4)
    for _ in range(2):
        pa, pb = a.draw(16, 224, 224), b.draw(16, 224, 224)
        assert set(pa) == set(pb)
        for k in pa:
            assert (pa[k] is None and pb[k] is None) or torch.equal(pa[k], pb[k]), k
