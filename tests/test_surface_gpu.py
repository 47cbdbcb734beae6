"""'HD' / 'ASD' on device (ctl_surface_stats / ctl_surface_map behind ops.surface_stats, ops.edt_sq, ops.surface_of and the device
branches of metrics.hd / hd_2D_stack / asd / surface_distances / runningMySegmentationScore.update).

Every expectation comes from the unchanged host (scipy) functions of metrics.py or from the rows the reference itself recorded in
tests/golden/io_cases.pt, never from the device code.  Bounds:
  * recorded rows: rtol 0, atol 1e-12, the project's figure for these columns (tests/test_kernels_gpu.py);
  * squared-distance maps, unit sampling: bit-equal (every value is an integer far below 2^53);
  * squared-distance maps, anisotropic sampling: relative 1e-12 (the two sides differ by the rounding of at most three products and two
    sums and possibly another equidistant feature: a few units of 2^-53);
  * HD / ASD of a volume: |dev - host| <= 1e-12 * max(1, |host|) (ASD: a mean of N <= 2.6e6 fp64 values summed as a tree on both sides has
    a relative error of about log2(N) * 2^-53 = 2.5e-15; HD: the rounding inside one d^2); HD with unit sampling: bit-equal."""
import os

import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import metrics, ops
from cooperative_training_and_latent_space_data_augmentation_amd.metrics import runningMySegmentationScore

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPACING = (10.0, 1.25, 1.25)


def phantom(d, h, w, jitter, seed, n_labels=3):
    """Concentric ellipses around a per-slice jittered centre: labels 1 / 2 / 3 where r < 0.30 / 0.22 / 0.15 * H * s."""
    rng = np.random.RandomState(seed)
    vol = np.zeros((d, h, w), dtype=np.int64)
    y, x = np.mgrid[0:h, 0:w]
    for z in range(d):
        cy, cx = h / 2 + rng.uniform(-jitter, jitter), w / 2 + rng.uniform(-jitter, jitter)
        r = np.hypot(y - cy, (x - cx) / 1.2)
        s = 1 - 0.5 * abs(z - d / 2) / d
        for lab, frac in ((1, 0.30), (2, 0.22), (3, 0.15))[:n_labels]:
            vol[z][r < frac * h * s] = lab
    return vol


def pair(d, h, w):
    return phantom(d, h, w, 6, 1).astype(np.uint8), phantom(d, h, w, 3, 0)          # prediction, ground truth


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, want):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


def rows_match(got, want, metrics_list, exact_hd=False):
    assert got[0] == want[0] and len(got) == len(want)
    for k, (g, w_) in enumerate(zip(got[1:], want[1:])):
        m = metrics_list[k % len(metrics_list)]
        print("  %-5s device %.17g host %.17g diff %.3g" % (m, g, w_, abs(g - w_)))
        if m == "Dice" or (m == "HD" and exact_hd):
            assert g == w_, (k, m, g, w_)
        else:
            assert close(g, w_), (k, m, g, w_)


def both_updates(pr, gt, spacing, foreground_only=False, n=4, metrics_list=("Dice", "HD", "ASD"), exact_hd=False):
    """update() with device volumes against update() with the same volumes as numpy arrays."""
    host = runningMySegmentationScore(n, metrics_list=list(metrics_list), foreground_only=foreground_only)
    devs = runningMySegmentationScore(n, metrics_list=list(metrics_list), foreground_only=foreground_only)
    want = host.update("p", pr, gt, voxel_spacing=spacing)
    got = devs.update("p", dev(pr), dev(gt), voxel_spacing=spacing)
    rows_match(got, want, list(metrics_list), exact_hd)
    return got, want


# ------------------------------------------------------------------------------------------------ 1. the reference's recorded rows
def _surface_cases():
    return torch.load(os.path.join(GOLDEN, "io_cases.pt"), weights_only=False)["surface_scores"]


def test_recorded_rows_through_update():
    for r in _surface_cases():
        ms = runningMySegmentationScore(4, idx2cls_dict=None if r["foreground_only"] else r["idx2cls"],
                                        metrics_list=["Dice", "HD", "ASD"], foreground_only=r["foreground_only"])
        for k, ((pr, gt), row) in enumerate(zip(r["volumes"], r["rows"])):
            got = ms.update("s%d" % k, pr.cuda(), gt.cuda(), voxel_spacing=r["spacing"])
            print(got, row)
            assert np.allclose(got[1:], row[1:], rtol=0, atol=1e-12)


def test_recorded_rows_through_free_functions():
    for r in _surface_cases():
        classes = [1] if r["foreground_only"] else [c for c in r["idx2cls"] if c > 0]
        for (pr, gt), row in zip(r["volumes"], r["rows"]):
            pr, gt = pr.cuda(), gt.cuda()
            for k, c in enumerate(classes):
                pm, gm = (pr > 0, gt > 0) if r["foreground_only"] else (pr == c, gt == c)
                got_hd = metrics.hd_2D_stack(pm, gm, pixelspacing=r["spacing"][:2], connectivity=2)
                got_asd = metrics.asd(pm, gm, voxelspacing=r["spacing"], connectivity=2)
                assert isinstance(got_hd, float) and isinstance(got_asd, float)
                assert np.allclose([got_hd, got_asd], row[1 + 3 * k + 1:1 + 3 * k + 3], rtol=0, atol=1e-12), (c, got_hd, got_asd, row)


# ------------------------------------------------------------------------------------------------ 2. surface and distance maps
SHAPES = [(1, 1, 1), (1, 37, 53), (7, 37, 53), (3, 64, 300), (2, 520, 70)]


def blob_mask(shape, seed):
    """Random blobs plus the phantom; every slice holds at least one voxel."""
    rng = np.random.RandomState(seed)
    d, h, w = shape
    m = phantom(d, h, w, 3, seed, n_labels=1) > 0
    seeds = rng.rand(*shape) < 0.01
    for dz, dy, dx in ((0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 0), (0, 2, 1)):      # small irregular blobs around the seeds
        m |= np.roll(seeds, (dz, dy, dx), axis=(0, 1, 2)) & (rng.rand(*shape) < 0.8)
    m[:, 0, 0] |= ~m.reshape(d, -1).any(axis=1)
    return m


def scipy_d2(mask, connectivity, sampling):
    """Squared distance of every voxel to the nearest voxel of metrics._border(mask), from scipy's feature indices."""
    from scipy.ndimage import distance_transform_edt
    idx = distance_transform_edt(~metrics._border(mask, connectivity), sampling=sampling, return_distances=False, return_indices=True)
    delta = np.indices(mask.shape) - idx
    if sampling is None:
        return (delta.astype(np.int64) ** 2).sum(axis=0).astype(np.float64)
    out = np.zeros(mask.shape, dtype=np.float64)
    for a, s in enumerate(sampling):
        out = out + (delta[a].astype(np.float64) * np.float64(s)) ** 2
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("connectivity", [1, 2])
def test_surface_and_distance_maps_vs_scipy(shape, connectivity):
    mask = blob_mask(shape, seed=sum(shape))
    md = dev(mask)
    # 3-D form
    assert torch.equal(ops.surface_of(md, connectivity).cpu(), torch.from_numpy(metrics._border(mask, connectivity)))
    assert np.array_equal(ops.edt_sq(md, None, connectivity).cpu().numpy(), scipy_d2(mask, connectivity, None))
    for sampling in ((10.0, 1.25, 1.25), (1.5, 1.25, 1.0)):
        got, want = ops.edt_sq(md, sampling, connectivity).cpu().numpy(), scipy_d2(mask, connectivity, sampling)
        rel = np.abs(got - want) / np.maximum(want, 1e-300)
        print(shape, connectivity, sampling, "3-D max rel", rel[want > 0].max() if (want > 0).any() else 0.0)
        assert np.all(np.abs(got - want) <= 1e-12 * want)
    # per-slice 2-D form
    want_surface = np.stack([metrics._border(s, connectivity) for s in mask])
    assert torch.equal(ops.surface_of(md, connectivity, per_slice=True).cpu(), torch.from_numpy(want_surface))
    assert torch.equal(ops.surface_of(md[0], connectivity).cpu(), torch.from_numpy(want_surface[0]))
    want = np.stack([scipy_d2(s, connectivity, None) for s in mask])
    assert np.array_equal(ops.edt_sq(md, None, connectivity, per_slice=True).cpu().numpy(), want)
    assert np.array_equal(ops.edt_sq(md[0], None, connectivity).cpu().numpy(), want[0])
    for sampling in ((1.25, 1.25), (1.5, 1.25), (1.0, 2.75)):
        got = ops.edt_sq(md, sampling, connectivity, per_slice=True).cpu().numpy()
        want = np.stack([scipy_d2(s, connectivity, sampling) for s in mask])
        assert np.all(np.abs(got - want) <= 1e-12 * want)


def test_connectivity_3_surface():
    mask = blob_mask((7, 37, 53), seed=5)
    assert torch.equal(ops.surface_of(dev(mask), 3).cpu(), torch.from_numpy(metrics._border(mask, 3)))
    assert np.array_equal(ops.edt_sq(dev(mask), None, 3).cpu().numpy(), scipy_d2(mask, 3, None))


def test_empty_mask_gives_inf_and_the_empty_flag():
    mask = np.zeros((3, 20, 30), dtype=bool)
    assert torch.isinf(ops.edt_sq(dev(mask), (2.0, 1.0, 1.0), 2)).all()
    assert not ops.surface_of(dev(mask), 2).any()
    mask[1, 5:9, 5:9] = True                                     # per-slice: slices 0 and 2 stay empty
    d2 = ops.edt_sq(dev(mask), None, 2, per_slice=True)
    assert torch.isinf(d2[0]).all() and torch.isinf(d2[2]).all() and torch.isfinite(d2[1]).all()
    pr, gt = mask.astype(np.uint8), np.zeros(mask.shape, dtype=np.int64)
    gt[1, 6:10, 6:10] = 1
    gt[2, 3, 3] = 1
    t = ops.surface_stats(dev(pr), dev(gt), 2, None, 2, "2d").cpu().numpy()          # [1, 2, 3, 4]
    assert t.shape == (1, 2, 3, 4)
    assert t[0, :, :, 3].tolist() == [[1.0, 0.0, 1.0], [1.0, 0.0, 1.0]]
    assert t[0, 0, :, 2].tolist() == [0.0, 12.0, 1.0] and t[0, 1, :, 2].tolist() == [0.0, 12.0, 0.0]      # sampled (other side's) surface voxels
    assert np.isinf(t[0, 0, 2, 0])                               # gt voxel of slice 2 has no predicted surface to measure to
    t3 = ops.surface_stats(dev(pr), dev(np.zeros_like(gt)), 2, None, 2, "3d").cpu().numpy()
    assert t3.shape == (1, 2, 1, 4) and t3[0, :, 0, 3].tolist() == [1.0, 1.0]


# ------------------------------------------------------------------------------------------------ 3. phantoms
@pytest.mark.parametrize("shape", [(10, 192, 192), (40, 256, 256)], ids=["10x192x192", "40x256x256"])
@pytest.mark.parametrize("foreground_only", [False, True], ids=["4class", "foreground"])
def test_phantom_update_device_vs_host(shape, foreground_only):
    pr, gt = pair(*shape)
    for c in (1, 2, 3):                                          # every class in every slice of both volumes: no HD term is skipped
        assert (pr == c).reshape(shape[0], -1).any(axis=1).all() and (gt == c).reshape(shape[0], -1).any(axis=1).all()
    both_updates(pr, gt, SPACING, foreground_only)
    both_updates(pr, gt, (1.0, 1.0, 1.0), foreground_only, exact_hd=True)


# ------------------------------------------------------------------------------------------------ 4. special cases
def _check_special(pr, gt, foreground_only=False, n=4):
    a = both_updates(pr, gt, (1.0, 1.0, 1.0), foreground_only, n=n, exact_hd=True)
    b = both_updates(pr, gt, SPACING, foreground_only, n=n)
    return a, b


def test_class_missing_from_some_predicted_slices():
    pr, gt = pair(10, 96, 96)
    pr[2][pr[2] == 3] = 2
    pr[7][pr[7] == 3] = 2
    pr[4][pr[4] == 1] = 0
    _check_special(pr, gt)
    t = ops.surface_stats(dev(pr), dev(gt), 4, SPACING[:2], 2, "2d").cpu().numpy()
    for c in (1, 2, 3):
        host_slices = sum(1 for p, g in zip(pr == c, gt == c) if p.sum() > 0 and g.sum() > 0)
        assert int((t[c - 1, 0, :, 3] == 0).sum()) == int((t[c - 1, 1, :, 3] == 0).sum()) == host_slices
    assert [int((t[c - 1, 0, :, 3] == 0).sum()) for c in (1, 2, 3)] == [9, 10, 8]


def test_class_missing_from_the_whole_prediction():
    pr, gt = pair(10, 96, 96)
    pr[pr == 3] = 2
    (got, want), _ = _check_special(pr, gt)
    assert got[1 + 3 * 2 + 1] == -1 and got[1 + 3 * 2 + 2] == 1e100 and want[1 + 3 * 2 + 1] == -1 and want[1 + 3 * 2 + 2] == 1e100


def test_mask_touching_all_six_faces_and_a_full_slice():
    pr, gt = pair(6, 40, 48)
    pr[:, 18:22, :] = 1
    pr[:, :, 20:24] = 1
    pr[2:4, 10:30, 10:30] = 1                                    # class 1 reaches every face of the volume
    gt[3] = 2                                                    # a mask that fills a whole slice
    gt[0, :, :] = np.where(gt[0] == 0, 1, gt[0])                 # no background left in slice 0
    _check_special(pr, gt)
    _check_special(pr, gt, foreground_only=True)
    full = np.ones((3, 17, 70), dtype=np.int64)
    _check_special(full.astype(np.uint8), full, n=2)


def test_single_voxel_objects_and_single_slice():
    pr, gt = np.zeros((5, 33, 65), dtype=np.uint8), np.zeros((5, 33, 65), dtype=np.int64)
    pr[1, 4, 60], gt[3, 30, 2] = 1, 1
    pr[0, 0, 0], gt[4, 32, 64] = 2, 2
    pr[2, 16, 30], gt[2, 16, 31] = 3, 3
    _check_special(pr, gt)
    p1, g1 = pair(1, 70, 130)                                    # D = 1
    _check_special(p1, g1)
    _check_special(p1, g1, foreground_only=True)
    one = np.ones((1, 1, 1), dtype=np.int64)
    _check_special(one.astype(np.uint8), one, n=2)


def test_ground_truth_labels_outside_the_classes():
    pr, gt = pair(6, 64, 64)
    gt[1, 10:20, 10:20] = 7
    gt[4, 30:34, 30:40] = -2
    gt[2][gt[2] == 2] = 255
    _check_special(pr, gt)


def test_free_functions_raise_on_empty_masks():
    full, empty = dev(phantom(3, 24, 24, 0, 0) > 0), dev(np.zeros((3, 24, 24), dtype=bool))
    for fn in (metrics.hd, metrics.surface_distances):
        for a, b in ((empty, full), (full, empty), (empty, empty)):
            with pytest.raises(RuntimeError) as dev_err:
                fn(a, b, (2.0, 1.0, 1.0), 2)
            with pytest.raises(RuntimeError) as host_err:
                fn(a.cpu().numpy(), b.cpu().numpy(), (2.0, 1.0, 1.0), 2)
            assert str(dev_err.value) == str(host_err.value)
    assert metrics.asd(empty, full) == 1e100 and metrics.asd(full, empty) == 1e100 and metrics.hd_2D_stack(full, empty) == -1


def test_free_functions_device_vs_host():
    pr, gt = pair(7, 50, 90)
    a, b = pr == 2, gt == 2
    for spacing, conn in ((None, 1), ((2.5, 1.25, 1.0), 1), ((2.5, 1.25, 1.0), 2), (1.5, 3)):
        assert close(metrics.hd(dev(a), dev(b), spacing, conn), metrics.hd(a, b, spacing, conn))
        assert close(metrics.asd(dev(a), dev(b), spacing, conn), metrics.asd(a, b, spacing, conn))
        sd = metrics.surface_distances(dev(a), dev(b), spacing, conn)
        want = metrics.surface_distances(a, b, spacing, conn)
        assert sd.is_cuda and sd.dtype == torch.float64 and tuple(sd.shape) == want.shape
        assert np.all(np.abs(sd.cpu().numpy() - want) <= 1e-12 * np.maximum(1.0, want))
    assert metrics.hd(dev(a), dev(b)) == metrics.hd(a, b)                                  # unit sampling: the same bits
    assert metrics.hd(dev(a[3]), dev(b[3]), (1.25, 1.0), 2) == pytest.approx(metrics.hd(a[3], b[3], (1.25, 1.0), 2), rel=1e-12, abs=0)
    spacing2 = (1.25, 1.5)
    assert close(metrics.hd_2D_stack(dev(a), dev(b), spacing2, 2), metrics.hd_2D_stack(a, b, spacing2, 2))


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_two_calls_give_the_same_bits():
    pr, gt = pair(10, 192, 192)
    prd, gtd = dev(pr), dev(gt)
    ms = runningMySegmentationScore(4, metrics_list=["Dice", "HD", "ASD"])
    first = ms.update("p", prd, gtd, voxel_spacing=SPACING)
    for _ in range(3):
        assert ms.update("p", prd, gtd, voxel_spacing=SPACING) == first
    t1 = ops.surface_stats(prd, gtd, 4, SPACING, 2, "3d")
    assert torch.equal(t1, ops.surface_stats(prd, gtd, 4, SPACING, 2, "3d"))


# ------------------------------------------------------------------------------------------------ 6. no volume leaves the device
def test_update_copies_no_volume_to_the_host(monkeypatch):
    shape = (10, 192, 192)
    pr, gt = pair(*shape)
    want = runningMySegmentationScore(4, metrics_list=["Dice", "HD", "ASD"]).update("p", pr, gt, voxel_spacing=SPACING)
    prd, gtd = dev(pr), dev(gt)
    limit = shape[1] * shape[2]
    # the tables read back: HD [3 classes, 2 sides, 10 slices, 4] + ASD [3, 2, 1, 4] = 264 doubles, and 2 * 4 * 4 counts
    assert 3 * 2 * shape[0] * 4 + 3 * 2 * 4 < limit

    def guarded(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.numel() >= limit:
                raise AssertionError("Tensor.%s of %d elements: a volume-sized host copy" % (name, self.numel()))
            return orig(self, *a, **k)
        return f
    for name in ("cpu", "numpy", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, guarded(name))
    with pytest.raises(AssertionError):
        prd.cpu()                                                # the guard is armed
    got = runningMySegmentationScore(4, metrics_list=["Dice", "HD", "ASD"]).update("p", prd, gtd, voxel_spacing=SPACING)
    monkeypatch.undo()
    rows_match(got, want, ["Dice", "HD", "ASD"])


def test_launches_per_update_do_not_depend_on_slices_or_classes():
    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
    counts = set()
    for shape, n in (((3, 40, 40), 2), ((10, 96, 96), 4), ((12, 64, 70), 9)):
        pr = dev(phantom(*shape, 3, 1).astype(np.uint8))
        gt = dev(phantom(*shape, 3, 0))
        ms = runningMySegmentationScore(n, metrics_list=["Dice", "HD", "ASD"])
        before = _ffi.lib.ctl_launch_count()
        ms.update("p", pr, gt, voxel_spacing=SPACING)
        counts.add(_ffi.lib.ctl_launch_count() - before)
    assert counts == {2 + 4 + 5}                                 # two confusion matrices, the per-slice form, the whole-volume form
