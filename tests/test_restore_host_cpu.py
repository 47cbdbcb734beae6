"""The numpy statements of the native-grid restoration (prepare.restore_scores_host / restore_labels_host / geometry) without a GPU:
against scipy.ndimage.map_coordinates at the same window coordinates, against the forward statements (crop / pad, resampling), and the
property the GPU comparison relies on: no fixture has a voxel whose two best classes are closer than the near-tie bound."""
import numpy as np
import pytest
from scipy import ndimage

from cooperative_training_and_latent_space_data_augmentation_amd import ops, prepare

import restore_cases as R

CASE_IDS = list(range(len(R.CASES)))


def _taps(s64, geo, order):
    """map_coordinates of every [Hc,Wc] plane of s64 [n,C,Hc,Wc] (or [n,Hc,Wc]) at the native voxels' window coordinates"""
    uy, ux, inside = prepare.restore_coordinates_host(geo)
    coords = np.stack(np.meshgrid(uy, ux, indexing="ij"))
    planes = s64.reshape((-1,) + s64.shape[-2:])
    out = np.stack([ndimage.map_coordinates(p, coords, order=order, mode="nearest") for p in planes])
    return out.reshape(s64.shape[:-2] + tuple(geo.native_hw)), inside


@pytest.mark.parametrize("index", CASE_IDS, ids=R.IDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_values_agree_with_map_coordinates(index, mode):
    geo = R.geometry_of(R.CASES[index])
    for c in R.CLASSES:
        s = R.scores_of(index, c).astype(np.float64)
        if mode == "prob":
            e = np.exp(s - s.max(axis=1, keepdims=True))
            s = e / e.sum(axis=1, keepdims=True)
        want, inside = _taps(s, geo, order=1)
        _, _, v, inside_h, _ = R.host_of(index, c, mode)
        assert np.array_equal(inside, inside_h) and v.shape == want.shape
        err = float(np.abs(v - want)[:, :, inside].max()) if inside.any() else 0.0
        print("  C=%d %s: %d outside, max |host - scipy| = %.3g" % (c, mode, int((~inside).sum()) * s.shape[0], err))
        assert err <= 1e-14
        outside = v[:, :, ~inside]
        assert np.all(outside[:, 1:] == 0) and np.all(outside[:, 0] == (1.0 if mode == "prob" else 0.0))


@pytest.mark.parametrize("index", CASE_IDS, ids=R.IDS)
def test_labels_agree_with_nearest_map_coordinates(index):
    case = R.CASES[index]
    geo = R.geometry_of(case)
    labels = np.random.default_rng(index).integers(0, 4, size=(case[0][0],) + tuple(geo.window_hw)).astype(np.uint8)
    got = prepare.restore_labels_host(labels, geo)
    assert got.dtype == np.uint8 and got.shape == (case[0][0],) + tuple(geo.native_hw)
    want, inside = _taps(labels.astype(np.float64), geo, order=0)
    uy, ux, _ = prepare.restore_coordinates_host(geo)
    off_half = lambda u: np.abs((u - np.floor(u)) - 0.5) > 1e-9                  # scipy's rounding of an exact half is its own
    clear = inside & off_half(uy)[:, None] & off_half(ux)[None, :]
    assert clear.sum() > 0.2 * inside.sum()                                       # q = 0.5 puts every second index on a half
    assert np.array_equal(got[:, clear], want[:, clear].astype(np.uint8))
    assert np.all(got[:, ~inside] == 0)


@pytest.mark.parametrize("index", CASE_IDS, ids=R.IDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_no_fixture_voxel_is_a_near_tie(index, mode):
    """the GPU tests compare labels where the host margin exceeds TIE * max |v|: that has to be every voxel"""
    for c in R.CLASSES:
        label, soft, v, inside, decided = R.host_of(index, c, mode)
        assert int((~decided).sum()) == 0, (c, int((~decided).sum()))
        assert label.dtype == np.uint8 and soft.dtype == np.float32 and np.all(label[:, ~inside] == 0)
        assert np.array_equal(label, np.where(inside[None], v.argmax(axis=1), 0))


def test_fixtures_cover_the_edge_rules():
    outside, low_band, past_end, both_ways = [], 0, 0, set()
    for case in R.CASES:
        geo = R.geometry_of(case)
        uy, ux, inside = prepare.restore_coordinates_host(geo)
        outside.append(int((~inside).sum()) * case[0][0])
        for a, u in ((0, uy), (1, ux)):
            c = np.arange(geo.native_hw[a]) * geo.q[a]
            low_band += int(((u >= -0.5) & (u < 0)).sum())
            past_end += int((c >= geo.resampled_hw[a] - 0.5).sum())
            both_ways.add(np.sign(geo.offset[a]))
            both_ways.add(2 if geo.q[a] > 1 else (-2 if geo.q[a] < 1 else 0))
    print("  outside voxels per case:", outside)
    assert min(outside) == 0 and max(outside) > 0 and low_band > 0 and past_end > 0
    assert both_ways >= {-1, 1, -2, 2, 0}                                       # cropped and padded, up- and down-sampled, identity


@pytest.mark.parametrize("index", [i for i in CASE_IDS if R.CASES[i][2] is None], ids=lambda i: R.IDS[i])
def test_identity_spacing_undoes_crop_or_pad(index):
    case = R.CASES[index]
    geo = R.geometry_of(case)
    assert geo.q == (1.0, 1.0) and geo.resampled_hw == geo.native_hw
    label = np.random.default_rng(7).integers(1, 4, size=case[0]).astype(np.uint8)       # no zeros: a lost voxel shows
    window = prepare._crop_or_pad_host(label, geo.window_hw)
    back = prepare.restore_labels_host(window, geo)
    _, _, inside = prepare.restore_coordinates_host(geo)
    assert np.array_equal(back[:, inside], label[:, inside]) and np.all(back[:, ~inside] == 0)
    ys, xs = np.arange(case[0][1]) - geo.offset[0], np.arange(case[0][2]) - geo.offset[1]
    kept = ((ys >= 0) & (ys < geo.window_hw[0]))[:, None] & ((xs >= 0) & (xs < geo.window_hw[1]))[None, :]
    assert np.array_equal(inside, kept)                                          # inside == what the crop kept
    scores = np.random.default_rng(8).normal(0, 3, size=(case[0][0], 4) + tuple(geo.window_hw)).astype(np.float32)
    lab, soft = prepare.restore_scores_host(scores, geo, want_soft=True)          # t == 0: the bits of the scores and their arg-max
    y0, x0 = np.clip(ys, 0, geo.window_hw[0] - 1), np.clip(xs, 0, geo.window_hw[1] - 1)
    picked = scores[:, :, y0][:, :, :, x0]
    assert np.array_equal(soft[:, :, inside].view(np.uint32), picked[:, :, inside].view(np.uint32))
    assert np.array_equal(lab[:, inside], picked.argmax(axis=1)[:, inside])


@pytest.mark.parametrize("index", CASE_IDS, ids=R.IDS)
def test_geometry_agrees_with_the_forward_statements(index):
    shape, spacing, new_spacing, window = R.CASES[index]
    geo = R.geometry_of(R.CASES[index])
    n, h, w = shape
    assert isinstance(geo, prepare.Geometry) and geo.native_hw == (h, w) and geo.spacing == tuple(float(v) for v in spacing)
    with pytest.raises(AttributeError):
        geo.q = (2.0, 2.0)
    if new_spacing is None:
        assert geo.resampled_hw == (h, w) and geo.q == (1.0, 1.0)
    else:
        nh, nw, r_h, r_w, identity = ops.resample_geometry(n, h, w, spacing, new_spacing)
        assert not identity and geo.resampled_hw == (nh, nw)
        assert geo.q == (spacing[1] / new_spacing[1], spacing[0] / new_spacing[0])
        assert abs(geo.q[0] * r_h - 1) < 1e-15 and abs(geo.q[1] * r_w - 1) < 1e-15
    assert geo.window_hw == (geo.resampled_hw if window is None else tuple(window))
    rh, rw = geo.resampled_hw
    ramp = (np.arange(rh)[:, None] * 1000 + np.arange(rw)[None, :] + 1)[None].astype(np.int64)       # value = 1000 y + x + 1, 0 = padding
    win = prepare._crop_or_pad_host(ramp, geo.window_hw)[0]
    jy, jx = np.nonzero(win)
    assert len(jy) and np.array_equal(win[jy, jx], (jy + geo.offset[0]) * 1000 + (jx + geo.offset[1]) + 1)      # the hs, ws of the crop
    image = np.zeros(shape, dtype=np.float32)
    pack = prepare.prepare_patient_host(image, np.zeros(shape, dtype=np.uint8), spacing=spacing, new_spacing=new_spacing, crop_size=window,
                                        normalize_2D=False)
    assert pack["image"].shape == (n, 1) + geo.window_hw and pack["label"].shape == (n,) + geo.window_hw
    assert prepare.restore_labels_host(pack["label"].astype(np.uint8), geo).shape == shape


def test_identity_by_the_sum_rule_and_bad_arguments():
    geo = prepare.geometry(2, 20, 24, (1.0, 1.0, 10.0), (1.00001, 1.00002, -1), (16, 16))       # upstream returns the input: so does the record
    assert geo.q == (1.0, 1.0) and geo.resampled_hw == (20, 24) and geo.offset == (2, 4)
    assert prepare.geometry(1, 9, 9, crop_size=(12, 12)).offset == (-2, -2)                      # floor((9 - 12) / 2), as ctl_crop_or_pad
    with pytest.raises(ValueError):
        prepare.geometry(2, 20, 24, None, (0.8, 0.8, -1), (16, 16))
    with pytest.raises(ValueError):
        prepare.restore_scores_host(np.zeros((2, 4, 8, 8), np.float32), geo)
    with pytest.raises(ValueError):
        prepare.restore_labels_host(np.zeros((2, 8, 8), np.uint8), geo)
    with pytest.raises(ValueError):
        prepare.restore_values_host(np.zeros((2, 4, 16, 16), np.float32), geo, mode="softmax")


@pytest.mark.parametrize("index", [i for i in CASE_IDS if R.CASES[i][2] is not None], ids=lambda i: R.IDS[i])
def test_round_trip_of_a_linear_ramp(index):
    """the inverse uses the forward statement's coordinates: a ramp a y + b x resampled forward (c = j r), cropped, and restored
    (c = i q) comes back where all four taps are real resampled samples"""
    shape, spacing, new_spacing, window = R.CASES[index]
    geo = R.geometry_of(R.CASES[index])
    n, h, w = shape
    ramp = np.broadcast_to((0.5 * np.arange(h)[:, None] + 0.25 * np.arange(w)[None, :] + 1.0).astype(np.float32), shape)
    fwd, _, _ = prepare.resample_inplane_host(ramp, spacing, new_spacing)
    win = prepare._crop_or_pad_host(fwd, geo.window_hw)
    v, inside = prepare.restore_values_host(win[:, None], geo)
    uy, ux, _ = prepare.restore_coordinates_host(geo)
    ok = inside.copy()
    for a, u, size in ((0, uy, h), (1, ux, w)):
        r = 1.0 / geo.q[a]
        valid = np.arange(geo.resampled_hw[a]) * r < size - 1                     # resampled samples the forward trip interpolated
        j0 = np.floor(u).astype(np.int64) + geo.offset[a]
        good = (u >= 0) & (u <= geo.window_hw[a] - 1) & (j0 >= 0) & (j0 + 1 < geo.resampled_hw[a])
        good &= valid[np.clip(j0, 0, geo.resampled_hw[a] - 1)] & valid[np.clip(j0 + 1, 0, geo.resampled_hw[a] - 1)]
        ok &= good[:, None] if a == 0 else good[None, :]
    assert ok.sum() > 0.1 * h * w
    err = np.abs(v[:, 0] - ramp)[:, ok].max()
    print("  %d voxels, max |restored - ramp| = %.3g" % (int(ok.sum()), err))
    assert err < 1e-5 * ramp.max()
