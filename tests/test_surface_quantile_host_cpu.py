"""Host (scipy / numpy) forms of the pooled surface-distance percentile: metrics.surface_distance_percentile, hd95, hd95_2D_stack, assd
and the 'HD95' / 'ASSD' columns of runningMySegmentationScore on numpy volumes.  Every expectation is the literal numpy statement of
the definition (np.percentile of the two hstack-ed surface_distances lists, np.mean of the two asd values, the slice loop)."""
import numpy as np
import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import metrics
from cooperative_training_and_latent_space_data_augmentation_amd.metrics import runningMySegmentationScore

SPACING = (10.0, 1.25, 1.25)
SHAPES = [(5, 40, 70), (7, 37, 53)]
_pairs = {}


def phantom(d, h, w, jitter, seed, n_labels=3):
    """The phantom of tests/test_surface_gpu.py: concentric ellipses around a per-slice jittered centre."""
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


def pair(shape):
    if shape not in _pairs:
        _pairs[shape] = (phantom(*shape, 6, 1).astype(np.uint8), phantom(*shape, 3, 0))          # prediction, ground truth
    return _pairs[shape]


def pooled(a, b, spacing, conn):
    return np.hstack((metrics.surface_distances(a, b, spacing, conn), metrics.surface_distances(b, a, spacing, conn)))


CASES = [(shape, c, conn, sp) for shape in SHAPES for c in (1, 2, 3) for conn in (1, 2) for sp in (None, SPACING)]


@pytest.mark.parametrize("shape,c,conn,spacing", CASES,
                         ids=["%s-c%d-conn%d-%s" % ("x".join(map(str, s)), c, k, "unit" if sp is None else "aniso") for s, c, k, sp in CASES])
def test_free_functions_equal_the_numpy_statements(shape, c, conn, spacing):
    pr, gt = pair(shape)
    a, b = pr == c, gt == c
    both = pooled(a, b, spacing, conn)
    got = metrics.hd95(a, b, spacing, conn)
    assert isinstance(got, float)
    assert got == np.percentile(both, 95)                                           # the same bits
    for q in (0, 50, 95, 97.5, 100):
        assert metrics.surface_distance_percentile(a, b, q, spacing, conn) == np.percentile(both, q), q
    assert metrics.surface_distance_percentile(a, b, 100, spacing, conn) == metrics.hd(a, b, spacing, conn)
    assert metrics.surface_distance_percentile(a, b, 0, spacing, conn) == both.min()
    assert got <= metrics.hd(a, b, spacing, conn)
    assert metrics.hd95(b, a, spacing, conn) == np.percentile(pooled(b, a, spacing, conn), 95)
    assert metrics.assd(a, b, spacing, conn) == np.mean((metrics.asd(a, b, spacing, conn), metrics.asd(b, a, spacing, conn)))
    sp2 = None if spacing is None else spacing[1:]
    vals = [np.percentile(pooled(r, g, sp2, conn), 95) for r, g in zip(a, b) if r.sum() > 0 and g.sum() > 0]
    assert len(vals) == shape[0]
    assert metrics.hd95_2D_stack(a, b, sp2, conn) == sum(vals) / len(vals)
    # identical masks: every distance is 0
    assert metrics.hd95(a, a, spacing, conn) == 0.0 and metrics.assd(a, a, spacing, conn) == 0.0
    assert metrics.hd95_2D_stack(a, a, sp2, conn) == 0.0 and metrics.surface_distance_percentile(a, a, 0, spacing, conn) == 0.0


def test_single_voxel_pair():
    a, b = np.zeros((3, 9, 11), dtype=bool), np.zeros((3, 9, 11), dtype=bool)
    a[0, 2, 3], b[2, 6, 6] = True, True
    for spacing in (None, SPACING):
        d = pooled(a, b, spacing, 1)
        assert d.size == 2 and d[0] == d[1]
        for q in (0, 50, 95, 100):
            assert metrics.surface_distance_percentile(a, b, q, spacing, 1) == np.percentile(d, q) == d[0]
    a2, b2 = a[0], np.zeros((9, 11), dtype=bool)
    b2[2, 3:5] = True                                                               # pooled n = 3: distances 0, 0 and 1
    assert metrics.hd95(a2, b2) == np.percentile(np.array([0.0, 0.0, 1.0]), 95)


def test_percentile_helper_is_numpys_on_random_lists():
    rng = np.random.RandomState(0)
    for trial in range(300):
        n = int(rng.randint(1, 400))
        d2 = np.sort(rng.randint(0, 500, n).astype(np.float64) * (1.0 if trial % 2 else 1.5625))
        for q in (0, 50, 95, 97.5, 100):
            k, k1, g = metrics._percentile_ranks(n, q)
            assert metrics._percentile_from_ranks(np.sqrt(d2[k]), np.sqrt(d2[k1]), g) == np.percentile(np.sqrt(d2), q), (n, q)
            assert metrics._percentile_from_table((d2[k], d2[k1], float(n), 0.0), q) == np.percentile(np.sqrt(d2), q)
    for bad in (-1, 100.5, float("nan")):
        with pytest.raises(ValueError):
            metrics._percentile_ranks(5, bad)


def test_empty_masks():
    full, empty = phantom(3, 24, 24, 0, 0) > 0, np.zeros((3, 24, 24), dtype=bool)
    for fn in (metrics.hd95, lambda a, b: metrics.surface_distance_percentile(a, b, 50)):
        for a, b in ((empty, full), (full, empty), (empty, empty)):
            with pytest.raises(RuntimeError) as err:
                fn(a, b)
            with pytest.raises(RuntimeError) as want:
                metrics.hd(a, b)
            assert str(err.value) == str(want.value)
    with pytest.raises(RuntimeError, match="first supplied array"):
        metrics.hd95(empty, full)
    with pytest.raises(RuntimeError, match="second supplied array"):
        metrics.hd95(full, empty)
    assert metrics.hd95_2D_stack(full, empty) == -1 and metrics.hd95_2D_stack(empty, full) == -1
    assert metrics.assd(empty, full) == 1e100 and metrics.assd(full, empty) == 1e100 and metrics.assd(empty, empty) == 1e100
    half = full.copy()
    half[1] = False                                                                 # only slices 0 and 2 hold both masks
    vals = [metrics.hd95(half[z], full[z]) for z in (0, 2)]
    assert metrics.hd95_2D_stack(half, full) == sum(vals) / 2
    with pytest.raises(ValueError):
        metrics.surface_distance_percentile(full, full, 101)


def test_score_table_on_numpy_volumes():
    names = ["Dice", "HD", "HD95", "ASD", "ASSD"]
    pr, gt = pair((5, 40, 70))
    ms = runningMySegmentationScore(4, metrics_list=names)
    assert ms.header == ["patient_id"] + ["%d_%s" % (c, m) for c in (1, 2, 3) for m in names]
    row = ms.update("p0", pr, gt, voxel_spacing=SPACING)
    assert row[0] == "p0" and len(row) == 1 + 3 * len(names)
    for c in (1, 2, 3):
        a, b = pr == c, gt == c
        want = [metrics.dice(a, b), metrics.hd_2D_stack(a, b, SPACING[:2], 2), metrics.hd95_2D_stack(a, b, SPACING[:2], 2),
                metrics.asd(a, b, SPACING, 2), metrics.assd(a, b, SPACING, 2)]
        assert row[1 + (c - 1) * 5:1 + c * 5] == want, c
        assert want[2] <= want[1]
    # the old names give what they gave without the new ones
    old = runningMySegmentationScore(4, metrics_list=["Dice", "HD", "ASD"]).update("p0", pr, gt, voxel_spacing=SPACING)
    assert old[1:] == [v for k, v in enumerate(row[1:]) if names[k % 5] in ("Dice", "HD", "ASD")]
    ms.update("p1", gt.astype(np.uint8), gt, voxel_spacing=SPACING)
    summary, rows, header = ms.get_scores()
    assert header == ms.header[1:] and len(rows[0]) == 15
    assert summary["2_HD95_mean"] == np.mean([row[1 + 5 + 2], 0.0]) and summary["3_ASSD_mean"] == np.mean([row[1 + 10 + 4], 0.0])
    fg = runningMySegmentationScore(4, metrics_list=names, foreground_only=True)
    frow = fg.update("p", pr, gt, voxel_spacing=SPACING)
    assert frow[3] == metrics.hd95_2D_stack(pr > 0, gt > 0, SPACING[:2], 2) and frow[5] == metrics.assd(pr > 0, gt > 0, SPACING, 2)
    with pytest.raises(ValueError):
        runningMySegmentationScore(4, metrics_list=["HD95"]).update("p", pr, gt)
    with pytest.raises(AssertionError):
        runningMySegmentationScore(4, metrics_list=["HD95"]).update("p", pr, gt, voxel_spacing=(1.0, 1.0, 5.0))


def test_unknown_metric_is_still_refused():
    for name in ("NSD", "hd95", "HD50"):
        with pytest.raises(NotImplementedError):
            runningMySegmentationScore(4, metrics_list=["Dice", name])
    assert runningMySegmentationScore.SUPPORTED == ("Dice", "VolError", "VolSim", "HD", "ASD", "HD95", "ASSD")
