"""Connected components and largest-component post-processing on device (ctl_cc_label / ctl_cc_keep_largest behind
ops.connected_components, ops.keep_largest_components, post_process.keep_largest_connected_components and the tester's `post_process`).

The oracle is scipy.ndimage.label on the host, built here from the definitions of include/ctl_hip.h ("connected components"), never from
the device code.  Every result is an integer, so every comparison is exact equality: there is no tolerance and no allowed share of
mismatches anywhere in this file."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from cooperative_training_and_latent_space_data_augmentation_amd import ops, post_process
from cooperative_training_and_latent_space_data_augmentation_amd.metrics import runningMySegmentationScore

pytestmark = pytest.mark.gpu

FORMS = [(True, 1), (True, 2), (False, 1), (False, 2), (False, 3)]          # (per_slice, connectivity): every allowed pair
FORM_IDS = ["2d-c1", "2d-c2", "3d-c1", "3d-c2", "3d-c3"]


# ---------------------------------------------------------------------------------------------- oracle
def _labels_of(arr, n, conn):
    idx = np.arange(arr.size, dtype=np.int64).reshape(arr.shape)
    out = np.full(arr.shape, -1, dtype=np.int32)
    for c in range(1, n):
        comp, k = ndimage.label(arr == c, structure=ndimage.generate_binary_structure(arr.ndim, conn))
        if k:
            first = np.asarray(ndimage.minimum(idx, comp, index=np.arange(1, k + 1))).astype(np.int32)
            inside = comp > 0
            out[inside] = first[comp[inside] - 1]
    return out


def _keep_of(arr, n, conn):
    """-> (kept, table [n - 1, 3]): scipy numbers components in C order of their first voxel, np.argmax takes the first largest."""
    idx = np.arange(arr.size, dtype=np.int64).reshape(arr.shape)
    kept, table = np.zeros(arr.shape, dtype=np.uint8), np.zeros((n - 1, 3), dtype=np.int64)
    for c in range(1, n):
        comp, k = ndimage.label(arr == c, structure=ndimage.generate_binary_structure(arr.ndim, conn))
        if k == 0:
            table[c - 1] = (0, 0, -1)
            continue
        sizes = np.bincount(comp.ravel(), minlength=k + 1)[1:]
        j = int(np.argmax(sizes)) + 1
        kept[comp == j] = c
        table[c - 1] = (k, sizes[j - 1], int(ndimage.minimum(idx, comp, index=j)))
    return kept, table


def oracle_labels(vol, n, conn, per_slice):
    if per_slice and vol.ndim == 3:
        return np.stack([_labels_of(s, n, conn) for s in vol])
    return _labels_of(vol, n, conn)


def oracle_keep(vol, n, conn, per_slice):
    if per_slice and vol.ndim == 3:
        parts = [_keep_of(s, n, conn) for s in vol]
        return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    kept, table = _keep_of(vol, n, conn)
    return kept, table[None]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_all(vol, n, conn, per_slice, what=""):
    """Labels, keep-largest and its table of one input against the oracle, voxel for voxel."""
    v = dev(vol)
    lab = ops.connected_components(v, n, connectivity=conn, per_slice=per_slice)
    kept, table = ops.keep_largest_components(v, n, connectivity=conn, per_slice=per_slice, want_table=True)
    assert lab.dtype == torch.int32 and kept.dtype == torch.uint8 and table.dtype == torch.int64
    assert lab.shape == v.shape and kept.shape == v.shape
    want_lab = oracle_labels(vol, n, conn, per_slice)
    want_kept, want_table = oracle_keep(vol, n, conn, per_slice)
    got_lab, got_kept, got_table = lab.cpu().numpy(), kept.cpu().numpy(), table.cpu().numpy()
    bad = int((got_lab != want_lab).sum())
    print("  %s %s n=%d conn=%d per_slice=%s: components %s, label mismatches %d, kept mismatches %d" % (
        what, vol.shape, n, conn, per_slice, want_table[..., 0].sum(axis=0).tolist(), bad, int((got_kept != want_kept).sum())))
    assert np.array_equal(got_lab, want_lab), (what, bad)
    assert np.array_equal(got_table, want_table), (what, got_table, want_table)
    assert np.array_equal(got_kept, want_kept), what
    assert np.array_equal(v.cpu().numpy(), vol)                     # the input is left alone
    return got_lab, got_kept, got_table


# ---------------------------------------------------------------------------------------------- inputs
def phantom(shape, n, seed, salt=0.01):
    """Concentric ellipses around a per-slice jittered centre, label c inside radius ~ (n - c) / (n - 1), plus salt noise: a fraction
    `salt` of the voxels takes a random value in [0, n + 1], so now and then one that is >= n."""
    d, h, w = shape
    rng = np.random.RandomState(seed)
    vol = np.zeros(shape, dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    for z in range(d):
        cy, cx = (h - 1) / 2 + rng.uniform(-3, 3), (w - 1) / 2 + rng.uniform(-3, 3)
        r = np.hypot((y - cy) / max(h, 2), (x - cx) / max(w, 2) / 1.2)
        s = 1 - 0.5 * abs(z - d / 2) / d
        for c in range(1, n):
            vol[z][r < 0.45 * s * (n - c) / (n - 1)] = c
    hit = rng.rand(*shape) < salt
    vol[hit] = rng.randint(0, n + 2, size=int(hit.sum()))
    return vol


def serpentine(h, w):
    """A one-voxel-wide path that fills the slice: full even rows joined at alternating ends."""
    a = np.zeros((h, w), dtype=np.uint8)
    a[0::2] = 1
    for y in range(1, h, 2):
        a[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return a


def spiral(h, w):
    """A one-voxel-wide square spiral from the corner to the centre."""
    a = np.zeros((h, w), dtype=np.uint8)
    y = x = d = turns = 0
    a[0, 0] = 1
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
    inside = lambda yy, xx: 0 <= yy < h and 0 <= xx < w
    while turns < 2:
        dy, dx = steps[d]
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and a[ny, nx] == 0 and (not inside(my, mx) or a[my, mx] == 0):
            y, x, turns = ny, nx, 0
            a[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return a


def structural_cases():
    cases = {}
    cases["serpentine"] = np.stack([serpentine(256, 256), serpentine(256, 256).T * 2, serpentine(256, 256)[::-1] * 3])
    cases["spiral"] = np.stack([spiral(256, 256), spiral(256, 256)[:, ::-1] * 2])
    z, y, x = np.indices((3, 256, 256))
    cases["checkerboard"] = ((z + y + x) % 2).astype(np.uint8)                       # class 1 against background
    cases["checkerboard two classes"] = (1 + (z + y + x) % 2).astype(np.uint8)
    cases["one class throughout"] = np.full((3, 70, 200), 3, dtype=np.uint8)
    absent = phantom((4, 96, 96), 4, 7)
    absent[absent == 2] = 0
    cases["absent class"] = absent
    cases["empty"] = np.zeros((2, 40, 70), dtype=np.uint8)
    b = np.zeros((2, 48, 200), dtype=np.uint8)                                        # tiles are 16 rows x 64 columns
    b[0, 5, 60:64], b[0, 5, 64:70] = 1, 1                                             # touch across the column border 63 | 64 only
    b[0, 12:16, 100], b[0, 16:20, 100] = 2, 2                                         # across the row border 15 | 16 only
    b[0, 30, 120:128], b[0, 30, 129:140] = 1, 1                                       # a gap next to the border 127 | 128: two components
    b[0, 40, 60:64], b[0, 41, 64:70] = 3, 3                                           # diagonal across the column border
    b[1, 15, 10:20], b[1, 16, 20:30] = 3, 3                                           # diagonal across the row border
    b[1, 31, 191], b[1, 32, 192] = 1, 1                                               # diagonal across a tile corner
    b[1, 32, 63], b[1, 31, 64] = 2, 2                                                 # the other diagonal across a tile corner
    cases["tile borders"] = b
    s = np.zeros((4, 40, 90), dtype=np.uint8)
    s[0, 10:20, 10:20], s[1, 19:30, 19:30] = 1, 1                                     # share the column (19, 19) only: a face across slices
    s[2, 30, 29] = 1                                                                  # (dz, dy, dx) = (1, 1, 0) from (1, 29, 29): connectivity 2
    s[2, 18, 18] = 1                                                                  # (1, -1, -1) from (1, 19, 19): connectivity 3
    s[1, 5, 60:70], s[2, 5, 70:80], s[3, 6, 80:85] = 2, 2, 2                          # edge contacts over the tile border at x = 64
    s[0, 35, 5:9], s[3, 35, 5:9] = 3, 3                                               # same place, two slices apart: never connected
    cases["slice boundaries"] = s
    g = np.zeros((2, 140, 140), dtype=np.uint8)
    i = np.arange(0, 130)
    g[0, i, i] = 1                                                                    # staircase across every tile border
    g[0, i, 135 - i] = 2
    g[1, 2 * (i // 2), i] = 3                                                         # steps of two
    g[1, 100:110, 5:15] = 1
    g[1, 110:120, 15:25] = 1                                                          # corner contact
    cases["diagonals"] = g
    t = np.zeros((3, 60, 150), dtype=np.uint8)
    t[0, 30:34, 2:6], t[0, 5:9, 100:104] = 1, 1                                       # two squares of 16: the one at (5, 100) starts first
    t[1, 5:9, 100:104], t[1, 30:34, 2:6] = 2, 2
    t[2, 50:52, 140:148], t[0, 40:44, 60:64] = 3, 3                                   # equal sizes in different slices
    t[2, 0, 0:3], t[2, 2, 0:3], t[2, 4, 0:3], t[2, 6, 0:2] = 1, 1, 1, 1               # three of three and a smaller one
    cases["tie"] = t
    o = phantom((3, 64, 130), 4, 11, salt=0.03)
    o[0, 3:9, 3:9], o[1, 20:30, 60:70], o[2, 0, :] = 4, 7, 255                        # values >= n_class split what they cut
    cases["values above n_class"] = o
    return cases


STRUCTURAL = structural_cases()


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 37, 53), (7, 37, 53), (3, 11, 150), (10, 192, 192)], ids=str)
def test_phantoms_match_scipy(shape, form):
    per_slice, conn = form
    for n in (2, 4, 8):
        for seed in (0, 1, 2):
            check_all(phantom(shape, n, seed, salt=0.05 if seed == 2 else 0.01), n, conn, per_slice, "phantom seed %d" % seed)
    for fill in (0, 1):
        check_all(np.full(shape, fill, dtype=np.uint8), 2, conn, per_slice, "constant %d" % fill)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_large_phantom_matches_scipy(form):
    per_slice, conn = form
    shape = (40, 256, 256)
    for n, seed, salt in ((4, 0, 0.002), (4, 1, 0.01), (2, 2, 0.01), (8, 3, 0.002)):
        check_all(phantom(shape, n, seed, salt), n, conn, per_slice, "phantom seed %d" % seed)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("case", sorted(STRUCTURAL))
def test_structural_cases_match_scipy(case, form):
    per_slice, conn = form
    check_all(STRUCTURAL[case], 4, conn, per_slice, case)


def test_tie_rule_is_exercised():
    """The constructed tie really is one (two components of the largest size), and the first in C order is the one kept."""
    t = STRUCTURAL["tie"]
    _, kept, table = check_all(t, 4, 1, True, "tie")
    assert table[0, 0].tolist() == [2, 16, 5 * 150 + 100] and kept[0, 5:9, 100:104].all() and not kept[0, 30:34, 2:6].any()
    assert table[2, 0].tolist() == [4, 3, 0]
    _, kept, table = check_all(t, 4, 1, False, "tie")
    assert table[0, 2].tolist() == [2, 16, 40 * 150 + 60] and kept[0, 40:44, 60:64].all() and not kept[2, 50:52, 140:148].any()


def test_two_dimensional_input_and_shapes():
    a = phantom((1, 50, 77), 4, 5, salt=0.03)[0]
    for conn in (1, 2):
        lab = ops.connected_components(dev(a), 4, connectivity=conn)
        assert lab.shape == (50, 77) and np.array_equal(lab.cpu().numpy(), _labels_of(a, 4, conn))
        kept, table = ops.keep_largest_components(dev(a), 4, connectivity=conn, want_table=True)
        want, want_table = _keep_of(a, 4, conn)
        assert kept.shape == (50, 77) and np.array_equal(kept.cpu().numpy(), want) and np.array_equal(table.cpu().numpy(), want_table[None])
    strided = dev(phantom((4, 40, 80), 4, 6, salt=0.03))[:, ::2, ::2]                 # a non-contiguous view is copied, not misread
    want, _ = oracle_keep(strided.cpu().numpy(), 4, 1, False)
    assert np.array_equal(ops.keep_largest_components(strided, 4).cpu().numpy(), want)


def test_argument_errors():
    v = dev(phantom((2, 16, 16), 4, 0))
    for bad in (v.int(), v.long(), v.float(), v.bool()):
        with pytest.raises(TypeError):
            ops.connected_components(bad, 4)
        with pytest.raises(TypeError):
            ops.keep_largest_components(bad, 4)
    with pytest.raises(ValueError):
        ops.connected_components(v[None], 4)
    with pytest.raises(ValueError):
        ops.keep_largest_components(v, 4, out=torch.empty((2, 16, 16), dtype=torch.int32, device="cuda"))
    from cooperative_training_and_latent_space_data_augmentation_amd._ffi import CtlError
    for kw in (dict(n_class=1), dict(n_class=256), dict(n_class=4, connectivity=0), dict(n_class=4, connectivity=3, per_slice=True),
               dict(n_class=4, connectivity=4)):
        with pytest.raises(CtlError):
            ops.connected_components(v, **kw)
        with pytest.raises(CtlError):
            ops.keep_largest_components(v, **kw)
    with pytest.raises(CtlError):
        ops.connected_components(v.cpu(), 4)


# ---------------------------------------------------------------------------------------------- aliasing, repeatability, streams, graphs
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_alias_repeat_and_stream_give_the_same_bits(form):
    per_slice, conn = form
    for vol in (phantom((7, 100, 130), 4, 3, salt=0.02), STRUCTURAL["serpentine"], STRUCTURAL["checkerboard two classes"]):
        v = dev(vol)
        lab1 = ops.connected_components(v, 4, connectivity=conn, per_slice=per_slice)
        kept1, table1 = ops.keep_largest_components(v, 4, connectivity=conn, per_slice=per_slice, want_table=True)
        lab2 = ops.connected_components(v, 4, connectivity=conn, per_slice=per_slice)
        kept2, table2 = ops.keep_largest_components(v, 4, connectivity=conn, per_slice=per_slice, want_table=True)
        assert torch.equal(lab1, lab2) and torch.equal(kept1, kept2) and torch.equal(table1, table2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lab3 = ops.connected_components(v, 4, connectivity=conn, per_slice=per_slice)
            kept3, table3 = ops.keep_largest_components(v, 4, connectivity=conn, per_slice=per_slice, want_table=True)
        side.synchronize()
        assert torch.equal(lab1, lab3) and torch.equal(kept1, kept3) and torch.equal(table1, table3)
        alias = v.clone()
        back = ops.keep_largest_components(alias, 4, connectivity=conn, per_slice=per_slice, out=alias)
        assert back is alias and torch.equal(alias, kept1)
        want, _ = oracle_keep(vol, 4, conn, per_slice)
        assert np.array_equal(kept1.cpu().numpy(), want)


@pytest.mark.parametrize("form", [(True, 1), (False, 1), (False, 3)], ids=["2d-c1", "3d-c1", "3d-c3"])
def test_launch_sequence_does_not_depend_on_the_content(form):
    """The call is captured ONCE into a graph on a phantom; the static input is then overwritten with the serpentine and with the
    checkerboard and the same graph replayed: every replay equals the oracle of the new content, and the launch census of an eager call
    is the same for all three.  (The graph is a single chain of kernels.)"""
    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
    per_slice, conn = form
    shape = (3, 256, 256)
    inputs = {"phantom": phantom(shape, 4, 0, salt=0.01), "serpentine": STRUCTURAL["serpentine"], "checkerboard": STRUCTURAL["checkerboard"]}
    static = dev(inputs["phantom"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside the capture
        ops.keep_largest_components(static, 4, connectivity=conn, per_slice=per_slice, want_table=True)
        ops.connected_components(static, 4, connectivity=conn, per_slice=per_slice)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kept, table = ops.keep_largest_components(static, 4, connectivity=conn, per_slice=per_slice, want_table=True)
        lab = ops.connected_components(static, 4, connectivity=conn, per_slice=per_slice)
    census = set()
    for name in ("serpentine", "checkerboard", "phantom"):
        static.copy_(dev(inputs[name]))
        graph.replay()
        torch.cuda.synchronize()
        want_kept, want_table = oracle_keep(inputs[name], 4, conn, per_slice)
        assert np.array_equal(kept.cpu().numpy(), want_kept), name
        assert np.array_equal(table.cpu().numpy(), want_table), name
        assert np.array_equal(lab.cpu().numpy(), oracle_labels(inputs[name], 4, conn, per_slice)), name
        before = _ffi.lib.ctl_launch_count()
        ops.keep_largest_components(static, 4, connectivity=conn, per_slice=per_slice, want_table=True)
        mid = _ffi.lib.ctl_launch_count()
        ops.connected_components(static, 4, connectivity=conn, per_slice=per_slice)
        census.add((int(mid - before), int(_ffi.lib.ctl_launch_count() - mid)))
    assert census == {(5, 3)}, census


# ---------------------------------------------------------------------------------------------- post_process, tester
@pytest.mark.parametrize("shape", [(64, 90), (5, 64, 90), (1, 1, 1)], ids=str)
def test_post_process_device_and_host_branch_agree(shape):
    for n in (2, 4):
        for seed in (0, 1):
            vol = phantom(shape if len(shape) == 3 else (1,) + shape, n, seed, salt=0.03).reshape(shape)
            got = post_process.keep_largest_connected_components(dev(vol), n)
            want = post_process.keep_largest_connected_components(vol, n)
            assert got.is_cuda and got.dtype == torch.uint8 and want.dtype == np.uint8
            assert np.array_equal(got.cpu().numpy(), want)
    t = STRUCTURAL["tie"]
    assert np.array_equal(post_process.keep_largest_connected_components(dev(t), 4).cpu().numpy(),
                          post_process.keep_largest_connected_components(t, 4))


class _VolumeSet:
    """The slice of the reference dataset interface the patient-wise tester reads (the stub of tests/test_engine_gpu.py)."""
    formalized_label_dict = {0: "BG", 1: "LV", 2: "MYO", 3: "RV"}

    def __init__(self, volumes):
        self.volumes, self.patient_number, self._cur = volumes, len(volumes), None

    def get_patient_data_for_testing(self, i, crop_size=None):
        self._cur = i
        return {"image": self.volumes[i][0], "label": self.volumes[i][1]}

    def get_id(self):
        return "patient%03d" % self._cur

    def get_voxel_spacing(self):
        return [10.0, 1.25, 1.25]


def _same_rows(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra[0] == rb[0] and len(ra) == len(rb)
        for x, y in zip(ra[1:], rb[1:]):
            assert x == y or (np.isnan(x) and np.isnan(y)), (ra, rb)


def test_tester_post_process_scores_the_post_processed_volume():
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import TestSegmentationNetwork, predict_volume
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()
    gen = torch.Generator().manual_seed(3)
    volumes = []
    for d in (6, 9):
        label = torch.from_numpy(phantom((d, 64, 64), 4, d, salt=0.0).astype(np.int64))
        image = (label.float() / 3 + 0.35 * torch.rand(d, 64, 64, generator=gen)).unsqueeze(1)
        volumes.append((image, label))
    data = _VolumeSet(volumes)
    mlist = ("Dice", "HD", "ASD")
    spacing = data.get_voxel_spacing()

    def run(**kw):
        t = TestSegmentationNetwork(data, crop_size=None, segmentation_model=solver, metrics_list=mlist, **kw)
        t.run()
        return t

    plain, none = run(), run(post_process=None)
    _same_rows(plain.segmentation_metric.tables, none.segmentation_metric.tables)
    raw = [predict_volume(solver, im.cuda(), chunk=10).cpu().numpy() for im, _ in volumes]
    for i, r in enumerate(raw):
        assert np.array_equal(none.result_dict["patient%03d" % i]["pred"], r)
    for key, per_slice in (("largest_cc", False), ("largest_cc_2d", True)):
        got = run(post_process=key)
        want = runningMySegmentationScore(4, idx2cls_dict=data.formalized_label_dict, metrics_list=list(mlist))
        changed = 0
        for i, (r, (_, label)) in enumerate(zip(raw, volumes)):
            host = np.stack([post_process.keep_largest_connected_components(s, 4) for s in r]) if per_slice \
                else post_process.keep_largest_connected_components(r, 4)
            changed += int((host != r).sum())
            assert np.array_equal(got.result_dict["patient%03d" % i]["pred"], host), (key, i)
            want.update("patient%03d" % i, dev(host), label.cuda(), voxel_spacing=spacing)
        print("  %s: %d voxels removed by the post-processing" % (key, changed))
        _same_rows(got.segmentation_metric.tables, want.tables)
        lean = run(post_process=key, keep_results=False)                              # the path without any full-volume copy
        _same_rows(lean.segmentation_metric.tables, want.tables)
        assert lean.result_dict == {}
