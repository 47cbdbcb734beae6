"""The four MR artefact corruptions on the device (csrc/ctl_corrupt.hip through ops and corrupt) against the fp64 host statements of
corrupt.py, which tests/test_corrupt_host_cpu.py pins to the literal spectrum edits.  The oracle is never the device code.

Bounds (from the number formats, not from what the kernels give; e = 2^-24, the unit roundoff of float32).
  axis operator   out[r,j] = sum over K = n L terms C[j,k] in[k].  The device multiplies the float32 rounding of C (relative e) into a
          float32 sum of K terms taken in any order (relative (K - 1) e to first order, one more e for a product that is not fused):
          |err| <= (K + 2) e sum_k |C[j,k]| |in[k]| per element, C and the sum in fp64.  The (K + 1)^2 e^2 term is below e for K < 4000.
  spike   The device evaluates the statement in fp64 and rounds once: e |want|.  Its fp64 part: sum(x) and X[k] are sums of N terms of
          size <= x, each with a product and a sincospi good to a few ulp: error <= (N + 8) 2^-53 S each, S = sum(x); they enter
          (m / N) ((A - Re X) cos + Im X sin) with |A - Re X| + |Im X| <= (intensity + 2) S and another 8 roundings: per pair
          2 (intensity + 2) (S / N) (N + 16) 2^-53, taken twice for the host statement's own rounding.
  bias    Coordinates have one rounding (t - h + 0.5 and h - 0.5 are exact).  A power p >= 1 of one carries (2 p - 1) e, at most 5 e for
          total degree 3, the three products of a term 3 e more, the running sum of 20 terms 20 e of M = sum |c| |u|^i |v|^j |w|^k: the
          polynomial is off by at most 28 e M (fused operations only round less); 32 e M with the second order.  exp turns that into a
          relative error (1.01: e^d - 1 <= 1.01 d for d < 0.01); expf is good to 1 ulp = 2 e (the ROCm device library's stated limit),
          the product with x rounds once more, and the fp64 reference rounds to float32 nowhere: |err| <= |want| 1.01 (32 M + 4) e.
  rigid   A source coordinate is a chain of three fused multiply-adds: each rounds a partial sum bounded by B_a = sum_b |M_ab| p_b + |o_a|,
          so it is off by at most 3 e B_a.  The interpolant of the zero-extended volume is continuous and piecewise linear, its slope
          along axis a at most G_a = the largest difference of neighbours along a (zeros included): a coordinate error moves the value by
          at most 3 e B_a G_a, whichever cell it lands in (s - floor(s) is exact).  Seven v0 + f (v1 - v0) in three levels, three
          roundings each on values within [-X, X], X = max |x|: at most 24 e X.  |err| <= 1.01 sum_a 3 e B_a G_a + 24 e X.
          An identity matrix gives coordinates and weights exactly: the copy equals x bit for bit.
  motion  The operator reads float32 copies that are off by the rigid bound R_t: sum_k |C_t[j,k]| R_t[k] on top of the operator bound,
          which is evaluated with |copy| + R_t for the copies.
  rescaled  (B + 3 Bmax) / (mx - mn) + 4 e per slice, the form tests/test_aug_bias_gpu.py uses: B the bound before the rescale, Bmax its
          maximum over the slice (minimum and maximum are off by at most Bmax each), mx - mn the slice's range.
"""
import os
import sys

import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, corrupt, ops

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.guarded import GuardedCall  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
E = 2.0 ** -24
SHAPES = [(1, 1, 1), (3, 5, 7), (5, 24, 20), (7, 33, 48)]
BIG = (10, 192, 192)
lib = _ffi.lib


def volume(shape, seed=0):
    """a smooth non-negative volume in [0, 1] with noise on top, float32"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in shape], indexing="ij")
    blob = np.exp(-2.0 * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2))
    return np.clip(0.7 * blob + 0.3 * rng.uniform(0, 1, shape), 0, 1).astype(F32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy().astype(np.float64)


def check(got, want, bound, what):
    err = np.abs(got - want)
    worst = float((err - bound).max())
    print(f"{what}: max err {err.max():.3g}, max bound {np.max(bound):.3g}, max (err - bound) {worst:.3g}")
    assert np.all(err <= bound), (what, float(err.max()), worst)


# ------------------------------------------------------------------------------------------------ axis operator
def operator_bound(volumes, matrix, axis):
    k = matrix.shape[1]
    return (k + 2) * E * corrupt.apply_operator_host([np.abs(v) for v in volumes], np.abs(matrix), axis)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_operator_random_matrix(shape, axis):
    """a dense random matrix over 1, 2 and 4 stacked volumes: every tile edge, every stride form"""
    rng = np.random.default_rng(axis)
    length = shape[axis]
    for n_vol in (1, 2, 4):
        vols = [volume(shape, 10 + t) - F32(0.25 * t) for t in range(n_vol)]
        c64 = rng.normal(size=(length, n_vol * length))
        c32 = c64.astype(F32)
        stack = dev(np.stack(vols[1:])) if n_vol > 1 else None
        got = host(ops.axis_operator(dev(vols[0]), dev(c32), axis, stack=stack))
        check(got, corrupt.apply_operator_host(vols, c64, axis), operator_bound(vols, c64, axis), f"operator {shape} axis {axis} x{n_vol}")


@pytest.mark.parametrize("shape", SHAPES + [BIG])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ghosting_matches_fp64(shape, axis):
    x = volume(shape, 1)
    cases = ((4, True, 0.75), (10, False, 0.5)) if shape != BIG else ((4, True, 0.75),)
    for num_ghosts, restore, intensity in cases:
        got = host(corrupt.ghosting(dev(x), num_ghosts, axis, intensity, restore))
        want = corrupt.ghosting_host(x, num_ghosts, axis, intensity, restore)
        c = corrupt.ghosting_operator(shape[axis], num_ghosts, intensity, restore)
        check(got, want, operator_bound([x], c, axis), f"ghosting {shape} axis {axis} n {num_ghosts} restore {restore}")
    pack = corrupt.ghosting(dev(x)[:, None], 4, axis, 0.75)                  # a tester pack [D,1,H,W] is viewed as the volume
    assert tuple(pack.shape) == shape and np.array_equal(host(pack), host(corrupt.ghosting(dev(x), 4, axis, 0.75)))


# ------------------------------------------------------------------------------------------------ spike
def spike_bound(x, want, n_pairs, intensity):
    n, s = x.size, float(x.astype(np.float64).sum())
    return E * np.abs(want) + 2 * n_pairs * 2 * (intensity + 2) * (s / n) * (n + 16) * 2.0 ** -53


def spike_positions(shape):
    shape = np.array(shape)
    centre = (shape // 2 + 0.5) / shape
    generic = np.array([0.31, 0.77, 0.12])
    return {"dc": [centre], "nyquist": [np.where(shape % 2 == 0, 0.0, centre)], "generic": [generic], "two": [generic, [0.9, 0.2, 0.6]]}


@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_spike_matches_fp64(shape):
    x = volume(shape, 2)
    for name, positions in spike_positions(shape).items():
        if shape == BIG and name not in ("generic", "two"):
            continue
        got = host(corrupt.spike(dev(x), positions, 2.5))
        want = corrupt.spike_host(x, positions, 2.5)
        n_pairs = len(corrupt.spike_wave_vectors(shape, positions)[1])
        check(got, want, spike_bound(x, want, n_pairs, 2.5), f"spike {shape} {name}")
        if name != "dc" and x.size > 1:
            assert not np.array_equal(got, x.astype(np.float64))


# ------------------------------------------------------------------------------------------------ bias
def bias_bound(shape, coef, want):
    u, v, w = (np.abs(corrupt.bias_coordinates(n)) for n in shape)
    m = np.zeros(shape)
    for c, (i, j, k) in zip(np.abs(np.asarray(coef, dtype=np.float64)), corrupt.BIAS_POWERS):
        m += c * (u[:, None, None] ** i) * (v[None, :, None] ** j) * (w[None, None, :] ** k)
    return np.abs(want) * 1.01 * (32 * m + 4) * E


@pytest.mark.parametrize("shape", SHAPES + [(4, 6, 8), BIG])
def test_bias_matches_fp64(shape):
    rng = np.random.default_rng(3)
    x = volume(shape, 3)
    for scale in (0.5, 0.0):
        coef = rng.uniform(-scale, scale, 20).astype(F32)
        got = host(corrupt.bias_field(dev(x), coef))
        want = corrupt.bias_field_host(x, coef)
        check(got, want, bias_bound(shape, coef, want), f"bias {shape} scale {scale}")
        if scale == 0.0:
            assert np.array_equal(got, x.astype(np.float64))                 # exp(0) = 1


# ------------------------------------------------------------------------------------------------ rigid copies and motion
def rigid_bound(x, matrices):
    """[T,D,H,W] the bound of the module docstring for every copy"""
    m = np.abs(np.asarray(matrices, dtype=F32).astype(np.float64)).reshape(-1, 3, 4)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in x.shape], indexing="ij"))
    pad = np.pad(x.astype(np.float64), 1)
    slope = [np.abs(np.diff(pad, axis=a)).max() for a in range(3)]
    out = np.zeros((m.shape[0],) + x.shape)
    for t in range(m.shape[0]):
        for a in range(3):
            reach = np.tensordot(m[t, a, :3], grid, axes=([0], [0])) + m[t, a, 3]
            out[t] += 1.01 * 3 * E * reach * slope[a]
    return out + 24 * E * np.abs(x).max()


def transforms(n_t, seed, angle=30.0):
    rng = np.random.default_rng(seed)
    degrees = rng.uniform(-angle, angle, (n_t, 3))
    degrees[0] = [angle, -angle, angle]                                     # the corners of the range
    return degrees, rng.uniform(-3.0, 3.0, (n_t, 3))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n_t", [1, 2, 3])
def test_rigid_copies_match_fp64(shape, n_t):
    x = volume(shape, 4)
    degrees, translations = transforms(n_t, n_t)
    for spacing in (None, (2.5, 1.25, 1.4)):
        m = corrupt.rigid_matrices(shape, spacing, degrees, translations)
        got = host(ops.corrupt_rigid3d(dev(x), m))
        check(got, corrupt.rigid3d_host(x, m), rigid_bound(x, m), f"rigid {shape} T {n_t} spacing {spacing}")
    m = corrupt.rigid_matrices(shape, (2.5, 1.25, 1.4), np.zeros((n_t, 3)), np.zeros((n_t, 3)))
    same = ops.corrupt_rigid3d(dev(x), m)
    assert torch.equal(same, dev(x).expand(n_t, *shape))                      # rotation 0: the input, exactly, through the gather
    m = corrupt.rigid_matrices(shape, None, np.zeros((1, 3)), [[1.0, -2.0, 3.0]])
    assert np.array_equal(host(ops.corrupt_rigid3d(dev(x), m)), corrupt.rigid3d_host(x, m))               # whole voxels: exact too


def motion_bound(x, copies_host, r_bound, matrix):
    vols = [np.abs(x.astype(np.float64))] + [np.abs(c) + r for c, r in zip(copies_host, r_bound)]
    moved = corrupt.apply_operator_host([np.zeros(x.shape)] + list(r_bound), np.abs(matrix), 2)
    return operator_bound(vols, matrix, 2) + moved


@pytest.mark.parametrize("shape,n_t", [(s, t) for s in SHAPES for t in (1, 2, 3)] + [(BIG, 2)])
def test_motion_matches_fp64(shape, n_t):
    x = volume(shape, 5)
    degrees, translations = transforms(n_t, 10 + n_t)
    times = np.sort(np.random.default_rng(n_t).uniform(0.1, 0.9, n_t))
    spacing = (2.5, 1.25, 1.4)
    got = host(corrupt.motion(dev(x), spacing, degrees, translations, times))
    want = corrupt.motion_host(x, spacing, degrees, translations, times)
    m = corrupt.rigid_matrices(shape, spacing, degrees, translations)
    bound = motion_bound(x, corrupt.rigid3d_host(x, m), rigid_bound(x, m), corrupt.motion_operator(shape[2], times))
    check(got, want, bound, f"motion {shape} T {n_t}")
    still = host(corrupt.motion(dev(x), spacing, np.zeros((n_t, 3)), np.zeros((n_t, 3)), times))         # nothing moved: the masks add up to one
    check(still, x.astype(np.float64), operator_bound([x] * (n_t + 1), corrupt.motion_operator(shape[2], times), 2), f"motion {shape} at rest")


# ------------------------------------------------------------------------------------------------ the whole corruption, rescaled
@pytest.mark.parametrize("kind", corrupt.KINDS)
def test_corrupt_volume_rescaled(kind):
    shape = (5, 24, 20)
    x = volume(shape, 6)
    for seed in (0, 1):
        p = corrupt.draw_parameters(kind, shape, np.random.default_rng(seed))
        raw_want = corrupt.corrupt_volume_host(x.astype(np.float64), kind, p, rescale=False).astype(np.float64)
        exact = {"RandomBias": lambda: corrupt.bias_field_host(x, p["coefficients"]),
                 "RandomSpike": lambda: corrupt.spike_host(x, p["positions"], p["intensity"]),
                 "RandomGhosting": lambda: corrupt.ghosting_host(x, p["num_ghosts"], p["axis"], p["intensity"], p["restore"]),
                 "RandomMotion": lambda: corrupt.motion_host(x, None, p["degrees"], p["translations"], p["times"])}[kind]()
        assert np.abs(raw_want - exact).max() <= E * np.abs(exact).max()      # corrupt_volume_host is that statement, rounded to float32
        if kind == "RandomBias":
            b = bias_bound(shape, np.asarray(p["coefficients"], dtype=F32), exact)
        elif kind == "RandomSpike":
            b = spike_bound(x, exact, len(corrupt.spike_wave_vectors(shape, p["positions"])[1]), p["intensity"])
        elif kind == "RandomGhosting":
            b = operator_bound([x], corrupt.ghosting_operator(shape[p["axis"]], p["num_ghosts"], p["intensity"], p["restore"]), p["axis"])
        else:
            m = corrupt.rigid_matrices(shape, None, p["degrees"], p["translations"])
            b = motion_bound(x, corrupt.rigid3d_host(x, m), rigid_bound(x, m), corrupt.motion_operator(shape[2], p["times"]))
        got_raw = host(corrupt.corrupt_volume(dev(x), kind, p, rescale=False))
        check(got_raw, exact, b, f"{kind} seed {seed}")
        mn, mx = exact.min(axis=(1, 2), keepdims=True), exact.max(axis=(1, 2), keepdims=True)
        want = (exact - mn) / ((mx - mn) + 1e-20)
        bound = (b + 3 * b.max(axis=(1, 2), keepdims=True)) / (mx - mn) + 4 * E
        got = corrupt.corrupt_volume(dev(x)[:, None], kind, p)
        assert tuple(got.shape) == (5, 1, 24, 20) and float(got.min()) == 0.0 and float(got.max()) == 1.0
        check(host(got)[:, 0], want, bound, f"{kind} seed {seed} rescaled")
        assert torch.equal(got, corrupt.corrupt_volume(dev(x)[:, None], kind, seed))                      # a seed is its draw


# ------------------------------------------------------------------------------------------------ bits, graphs, guard bands
def made(kind, shape, seed=0):
    p = corrupt.draw_parameters(kind, shape, np.random.default_rng(seed))
    if kind == "RandomSpike":
        p["positions"] = [[0.31, 0.77, 0.12], [0.9, 0.2, 0.6]]
    return corrupt.Corruption(kind, p, shape, spacing=(2.5, 1.25, 1.4))


@pytest.mark.parametrize("kind", corrupt.KINDS)
def test_two_calls_and_a_graph_replay_give_the_same_bits(kind):
    shape = (7, 33, 48)
    f = made(kind, shape)
    static = dev(volume(shape, 7))
    first = f(static).clone()
    assert torch.equal(f(static), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                           # warm-up outside the capture
        f(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out = torch.empty(shape, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f(static, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    other = dev(volume(shape, 8))
    static.copy_(other)                                                     # new content, the same launches
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, f(other)) and not torch.equal(out, first)
    before = lib.ctl_launch_count()
    f(static)
    assert int(lib.ctl_launch_count() - before) == {"RandomBias": 1, "RandomSpike": 2, "RandomGhosting": 1, "RandomMotion": 2}[kind]


@pytest.mark.parametrize("shape", [(3, 5, 7), (7, 33, 48)])
def test_written_buffers_between_guard_bands(shape):
    """every buffer a kernel writes, sized exactly and poisoned between guard bands; the inputs sized exactly too, so a read past their
    end meets the guard pattern (1.5e16 as a float) and shows in the comparison"""
    n = int(np.prod(shape))
    x = volume(shape, 9)

    def fill(values):
        return lambda buf: buf.flat().copy_(dev(values).reshape(-1))

    # bias
    coef = np.random.default_rng(0).uniform(-0.5, 0.5, 20).astype(F32)
    gc = GuardedCall("cuda")
    xin, out = gc.out("x", n, written=False, init=fill(x)), gc.out("out", n)
    launch = lambda: ops.corrupt_bias_field(xin.view(shape), coef, out=out.view(shape))
    gc.run(launch)
    check(host(out.view(shape)), corrupt.bias_field_host(x, coef), bias_bound(shape, coef, corrupt.bias_field_host(x, coef)), "guarded bias")
    gc.rerun(launch)
    # spike: the workspace is written completely, and nothing beside it
    k, mult = corrupt.spike_wave_vectors(shape, [[0.31, 0.77, 0.12], [0.9, 0.2, 0.6]])
    nbytes = lib.ctl_corrupt_spike_ws_bytes(*shape, len(mult))
    assert nbytes > 0 and nbytes % 8 == 0
    gc = GuardedCall("cuda")
    xin, out, ws = gc.out("x", n, written=False, init=fill(x)), gc.out("out", n), gc.out("ws", nbytes // 8, dtype=torch.float64)
    launch = lambda: ops.corrupt_spike(xin.view(shape), k, mult, 2.0, out=out.view(shape), workspace=ws.flat())
    gc.run(launch)
    want = corrupt.spike_host(x, [[0.31, 0.77, 0.12], [0.9, 0.2, 0.6]], 2.0)
    check(host(out.view(shape)), want, spike_bound(x, want, len(mult), 2.0), "guarded spike")
    gc.rerun(launch)
    # rigid copies, then the operator over x and the copies (axis 2), and over x alone along the outer axes
    degrees, translations = transforms(2, 1)
    m = corrupt.rigid_matrices(shape, None, degrees, translations)
    gc = GuardedCall("cuda")
    xin, copies = gc.out("x", n, written=False, init=fill(x)), gc.out("copies", 2 * n)
    launch = lambda: ops.corrupt_rigid3d(xin.view(shape), m, out=copies.view((2,) + shape))
    gc.run(launch)
    check(host(copies.view((2,) + shape)), corrupt.rigid3d_host(x, m), rigid_bound(x, m), "guarded rigid")
    gc.rerun(launch)
    stack_np = copies.view((2,) + shape).cpu().numpy()
    for axis, n_vol in ((2, 3), (1, 1), (0, 1)):
        length = shape[axis]
        c64 = np.random.default_rng(axis).normal(size=(length, n_vol * length))
        gc = GuardedCall("cuda")
        xin, out = gc.out("x", n, written=False, init=fill(x)), gc.out("out", n)
        cm = gc.out("matrix", c64.size, written=False, init=fill(c64.astype(F32)))
        st = gc.out("stack", (n_vol - 1) * n, written=False, init=fill(stack_np)) if n_vol > 1 else None
        launch = lambda: ops.axis_operator(xin.view(shape), cm.view(c64.shape), axis, out=out.view(shape),
                                           stack=None if st is None else st.view((n_vol - 1,) + shape))
        gc.run(launch)
        vols = [x] + ([stack_np[0], stack_np[1]] if n_vol > 1 else [])
        check(host(out.view(shape)), corrupt.apply_operator_host(vols, c64, axis), operator_bound(vols, c64, axis), f"guarded operator axis {axis}")
        gc.rerun(launch)


def test_python_layer_arguments():
    x = torch.zeros(2, 4, 6, device="cuda")
    with pytest.raises(ValueError):
        ops.corrupt_bias_field(x, np.zeros(19))
    with pytest.raises(ValueError):
        ops.axis_operator(x, torch.zeros(6, 12, device="cuda"), 2)          # a matrix for two volumes, one given
    with pytest.raises(ValueError):
        ops.axis_operator(x, torch.zeros(6, 6, device="cuda"), 3)
    with pytest.raises(ValueError):
        ops.corrupt_rigid3d(x.double(), np.eye(3, 4)[None])
    with pytest.raises(_ffi.CtlError, match="aliases"):
        ops.corrupt_bias_field(x, np.zeros(20), out=x)
    with pytest.raises(_ffi.CtlError, match="multiplicity"):
        ops.corrupt_spike(x, [[1, 1, 1]], [1], 2.0)
    strided = torch.rand(2, 4, 12, device="cuda")[:, :, ::2]                # copied, not misread
    assert torch.equal(ops.corrupt_bias_field(strided, np.zeros(20)), strided)


# ------------------------------------------------------------------------------------------------ through the tester
class _Patients:
    """The slice of the reference dataset interface the patient-wise tester reads, serving clean host packs."""
    formalized_label_dict = {0: "BG", 1: "LV", 2: "MYO", 3: "RV"}

    def __init__(self, n=2, shape=(6, 32, 32)):
        self.patient_number, self.shape, self._cur = n, shape, None

    def get_patient_data_for_testing(self, i, crop_size=None):
        self._cur = i
        d, h, w = self.shape
        y, x = np.mgrid[0:h, 0:w]
        r = np.hypot((y - h / 2) / h, (x - w / 2 + i) / w)
        label = np.zeros(self.shape, dtype=np.int64)
        for c, rad in ((3, 0.42), (2, 0.3), (1, 0.18)):
            label[:, r < rad] = c
        image = np.clip(label / 4.0 + 0.25 * np.random.default_rng(i).uniform(0, 1, self.shape), 0, 1).astype(F32)
        return {"image": torch.from_numpy(image[:, None]), "label": torch.from_numpy(label)}

    def get_id(self):
        return "patient%03d" % self._cur

    def get_voxel_spacing(self):
        return [10.0, 1.25, 1.25]


@pytest.mark.parametrize("kind", corrupt.KINDS)
def test_tester_scores_the_corrupted_dataset_like_the_host_corruption(kind):
    """CorruptedDataset through TestSegmentationNetwork, unchanged, against the tester fed the fp64 host corruption of the same draws.
    The two packs differ by the bounds above, so the logits differ a little and an arg-max can flip where two classes tie.  With d the
    largest difference between the two runs' logits, a voxel can flip only where the host run's two best logits are within 2 d: every
    differing voxel must be one of those, those must be rare (under 1 % of the volume: d is rounding noise, not a different image;
    test_corrupt_volume_rescaled bounds the difference of the packs), and a patient without a flipped voxel must have the very same
    Dice row."""
    from cooperative_training_and_latent_space_data_augmentation_amd.solver import AdvancedTripletReconSegmentationModel
    from cooperative_training_and_latent_space_data_augmentation_amd.tester import TestSegmentationNetwork
    torch.manual_seed(0)
    solver = AdvancedTripletReconSegmentationModel(network_type="FCN_16_standard", image_ch=1, num_classes=4, use_gpu=True)
    solver.eval()

    def run(host_side):
        ds = corrupt.CorruptedDataset(_Patients(), kind, n_augmented=2, seed=5, host=host_side)
        t = TestSegmentationNetwork(ds, crop_size=None, segmentation_model=solver, metrics_list=("Dice",))
        t.run()
        return t

    on_device, on_host = run(False), run(True)
    rows_d, rows_h = on_device.segmentation_metric.tables, on_host.segmentation_metric.tables
    assert [r[0] for r in rows_d] == [r[0] for r in rows_h] == ["patient000_0", "patient001_0", "patient000_1", "patient001_1"]
    clean = _Patients()
    for a, b in zip(rows_d, rows_h):
        pid = a[0]
        rd, rh = on_device.result_dict[pid], on_host.result_dict[pid]
        assert np.array_equal(rd["label"], rh["label"])
        assert np.array_equal(rd["label"], clean.get_patient_data_for_testing(int(pid[7:10]))["label"].numpy())        # labels untouched
        assert rd["image"].min() == 0 and rd["image"].max() == 1 and rh["image"].min() == 0 and rh["image"].max() == 1
        delta = float(np.abs(rd["soft_pred"] - rh["soft_pred"]).max())
        top = np.sort(rh["soft_pred"], axis=1)
        tie = (top[:, -1] - top[:, -2]) <= 2 * delta
        flipped = rd["pred"] != rh["pred"]
        print(f"{kind} {pid}: logit difference {delta:.3g}, {int(tie.sum())} tie voxel(s), {int(flipped.sum())} flipped")
        assert not np.any(flipped & ~tie) and tie.mean() < 0.01
        if not flipped.any():
            assert len(a) == len(b) and all(x == y or (np.isnan(x) and np.isnan(y)) for x, y in zip(a[1:], b[1:])), (a, b)
