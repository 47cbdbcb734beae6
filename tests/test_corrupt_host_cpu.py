"""The fp64 host statements of corrupt.py against independent restatements, without a GPU: the operator-matrix forms of ghosting and
motion and the plane-wave form of the spike equal the literal `fftshift(fftn)` -> edit -> `ifftn` -> real forms to 1e-12 (volumes in
[0, 1]: the FFT round trip itself is good to about 1e-15), the bias field equals a literal meshgrid polynomial; the parameter draws,
the centre-swap rule of the motion segments and the ids and counts of CorruptedDataset."""
import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import corrupt

SHAPES = [(1, 1, 1), (3, 5, 7), (5, 24, 20), (7, 33, 48)]
TOL = 1e-12


def volume(shape, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 1.0, shape)


def spectrum(x):
    return np.fft.fftshift(np.fft.fftn(x))


def image(s):
    return np.fft.ifftn(np.fft.ifftshift(s)).real


# ------------------------------------------------------------------------------------------------ ghosting
def ghosting_literal(x, num_ghosts, axis, intensity, restore):
    s = spectrum(x)
    mid = x.shape[axis] // 2
    sl = [slice(None)] * 3
    sl[axis] = mid
    kept = s[tuple(sl)].copy()
    pl = [slice(None)] * 3
    pl[axis] = slice(None, None, num_ghosts)
    s[tuple(pl)] *= 1 - intensity
    if restore:
        s[tuple(sl)] = kept
    return image(s)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ghosting_operator_is_the_spectrum_edit(shape, axis):
    x = volume(shape, 1)
    for num_ghosts, restore, intensity in ((4, True, 0.75), (10, False, 0.5), (7, True, 1.0)):
        got = corrupt.ghosting_host(x, num_ghosts, axis, intensity, restore)
        want = ghosting_literal(x, num_ghosts, axis, intensity, restore)
        assert np.abs(got - want).max() <= TOL, (shape, axis, num_ghosts, restore)
    c = corrupt.ghosting_operator(shape[axis], 4, 0.6, True)
    assert c.shape == (shape[axis], shape[axis]) and np.abs(c - c.T).max() <= 1e-15        # a real symmetric circulant


# ------------------------------------------------------------------------------------------------ motion
def motion_literal(x, copies, times):
    """TorchIO's add_artifact with the swap stated as: the spectrum of x goes where the segment holds the centre of the last axis."""
    spectra = [spectrum(v) for v in [x] + list(copies)]
    length = x.shape[2]
    ends = [int(v) for v in np.floor(length * np.asarray(times))] + [length]
    ini, centre = 0, None
    for i, fin in enumerate(ends):
        if ini <= length // 2 < fin:
            centre = i
        ini = fin
    spectra[0], spectra[centre] = spectra[centre], spectra[0]
    result = np.zeros_like(spectra[0])
    ini = 0
    for s, fin in zip(spectra, ends):
        result[..., ini:fin] = s[..., ini:fin]
        ini = fin
    return image(result)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n_t", [1, 2, 3])
def test_motion_operator_is_the_segmented_spectrum(shape, n_t):
    rng = np.random.default_rng(n_t)
    x = volume(shape, 2)
    degrees, translations = rng.uniform(-30, 30, (n_t, 3)), rng.uniform(-3, 3, (n_t, 3))
    times = np.sort(rng.uniform(0.05, 0.95, n_t))
    copies = corrupt.rigid3d_host(x, corrupt.rigid_matrices(shape, (1.0, 1.25, 1.5), degrees, translations))
    got = corrupt.motion_host(x, (1.0, 1.25, 1.5), degrees, translations, times)
    want = motion_literal(x, copies, times)
    assert np.abs(got - want).max() <= TOL, (shape, n_t)
    masks = corrupt.motion_segments(shape[2], times)
    assert masks.shape == (n_t + 1, shape[2]) and np.array_equal(masks.sum(axis=0), np.ones(shape[2]))     # a partition of the axis


def test_motion_centre_swap_rule():
    def owners(length, times):
        return corrupt.motion_segments(length, times).argmax(axis=0).tolist()

    # L = 20, centre 10.  times 0.52: floor(10.4) = 10, so [0, 10) does NOT hold the centre although 0.52 > 0.5
    assert owners(20, [0.52, 0.8]) == [1] * 10 + [0] * 6 + [2] * 4
    assert owners(20, [0.2, 0.4]) == [2] * 4 + [1] * 4 + [0] * 12                # the last segment holds it: x and copy 2 swap
    assert owners(20, [0.6, 0.9]) == [0] * 12 + [1] * 6 + [2] * 2                # the first one does: nothing moves
    assert owners(7, [0.5]) == [1] * 3 + [0] * 4                                 # odd: centre 3, floor(3.5) = 3
    assert owners(20, [0.5, 0.5]) == [2] * 10 + [0] * 10                         # an empty segment [10, 10) for copy 1...
    assert corrupt.motion_segments(20, [0.5, 0.5])[1].sum() == 0                 # ...which contributes nothing
    assert owners(1, [0.3]) == [0]
    with pytest.raises(ValueError):
        corrupt.motion_segments(20, [0.8, 0.2])


def test_rigid_matrices():
    m = corrupt.rigid_matrices((5, 24, 20), (10.0, 1.25, 1.4), np.zeros((2, 3)), np.zeros((2, 3)))
    assert np.array_equal(m, np.broadcast_to(np.eye(3, 4), (2, 3, 4)))          # exactly the identity
    x = volume((5, 24, 20), 3)
    assert np.array_equal(corrupt.rigid3d_host(x, m)[1], x)
    m = corrupt.rigid_matrices((5, 24, 20), None, [[0, 0, 0]], [[1.0, -2.0, 3.0]])            # a whole-voxel shift, zeros move in
    got = corrupt.rigid3d_host(x, m)[0]
    want = np.zeros_like(x)
    want[:4, 2:, :17] = x[1:, :22, 3:]
    assert np.abs(got - want).max() <= 1e-15
    m = corrupt.rigid_matrices((9, 9, 9), (2.0, 2.0, 2.0), [[0, 0, 90]], [[0, 0, 0]])[0]      # about axis 2: (i0, i1) -> (8 - i1, i0)
    assert np.abs(m[:, :3] @ np.array([1.0, 2.0, 5.0]) + m[:, 3] - np.array([6.0, 1.0, 5.0])).max() <= 1e-12
    r = corrupt.rigid_matrices((4, 6, 8), None, [[10, -20, 30]], [[0, 0, 0]])[0][:, :3]
    assert np.abs(r @ r.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(r) - 1) <= 1e-15


# ------------------------------------------------------------------------------------------------ spike
def spike_literal(x, positions, intensity):
    s = spectrum(x)
    shape = np.array(x.shape)
    amp = s.max() * intensity                                                   # numpy's complex max: the DC term of a non-negative volume
    assert amp.imag == 0 and abs(amp.real - intensity * x.sum()) <= 1e-9 * max(1.0, x.sum())
    mid = shape // 2
    out = s.copy()
    for pos in np.asarray(positions, dtype=np.float64).reshape(-1, 3):
        d = np.floor(pos * shape).astype(int) - mid
        out[tuple(mid + d)] = amp
        out[tuple((mid - d) % shape)] = amp
    return image(out)


def spike_cases(shape):
    shape = np.array(shape)
    centre = (shape // 2 + 0.5) / shape                                         # d = 0: the DC term itself
    nyquist = np.where(shape % 2 == 0, 0.0, centre)                             # index 0 of an even axis: d = -n / 2 == +n / 2
    generic = np.array([0.31, 0.77, 0.12])
    return {"dc": [centre], "nyquist": [nyquist], "generic": [generic], "two": [generic, [0.9, 0.2, 0.6]], "twice": [generic, generic],
            "mirrored": [generic, ((2 * (shape // 2) - np.floor(generic * shape)) % shape + 0.5) / shape]}


@pytest.mark.parametrize("shape", SHAPES + [(4, 6, 8)])
def test_spike_plane_wave_is_the_spectrum_edit(shape):
    x = volume(shape, 4)
    for name, positions in spike_cases(shape).items():
        got = corrupt.spike_host(x, positions, 2.5)
        want = spike_literal(x, positions, 2.5)
        assert np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max()), (shape, name)
    k, mult = corrupt.spike_wave_vectors(shape, spike_cases(shape)["nyquist"])
    assert mult.tolist() == [1] and len(corrupt.spike_wave_vectors(shape, spike_cases(shape)["twice"])[1]) == 1
    with pytest.raises(AssertionError):
        corrupt.spike_host(x - 2.0, [[0.3, 0.3, 0.3]], 1.0)


# ------------------------------------------------------------------------------------------------ bias
@pytest.mark.parametrize("shape", SHAPES + [(4, 6, 8)])
def test_bias_field_is_the_meshgrid_polynomial(shape):
    rng = np.random.default_rng(5)
    x = volume(shape, 5)
    coef = rng.uniform(-0.5, 0.5, 20).astype(np.float32)
    axes = []
    for n in shape:
        h = n // 2
        if n % 2 == 0:
            mesh = np.arange(-h, h) + 0.5                                       # TorchIO's mesh, one short on an odd axis
            axes.append(mesh / mesh.max())
        else:
            axes.append(np.zeros(n) if h == 0 else (np.arange(n) - h + 0.5) / (h - 0.5))
    u, v, w = np.meshgrid(*axes, indexing="ij")
    field, n = np.zeros(shape), 0
    for i in range(4):
        for j in range(4 - i):
            for k in range(4 - (i + j)):
                field += np.float64(coef[n]) * u ** i * v ** j * w ** k
                n += 1
    assert n == 20
    got = corrupt.bias_field_host(x, coef)
    assert np.abs(got - x * np.exp(field)).max() <= TOL * np.abs(got).max()
    assert np.array_equal(corrupt.bias_field_host(x, np.zeros(20)), x)


# ------------------------------------------------------------------------------------------------ draws
def test_draw_parameters_ranges_and_determinism():
    for kind in corrupt.KINDS:
        a = corrupt.draw_parameters(kind, (10, 192, 192), np.random.default_rng(7))
        b = corrupt.draw_parameters(kind, (10, 192, 192), np.random.default_rng(7))
        c = corrupt.draw_parameters(kind, (10, 192, 192), np.random.default_rng(8))
        assert isinstance(a, dict) and a == b and a != c, kind
    seen_axes, seen_ghosts = set(), set()
    for seed in range(200):
        rng = np.random.default_rng(seed)
        p = corrupt.draw_parameters("RandomBias", (4, 4, 4), rng)
        assert len(p["coefficients"]) == 20 and all(-0.5 <= v < 0.5 for v in p["coefficients"])
        p = corrupt.draw_parameters("RandomSpike", (4, 4, 4), rng)
        assert np.shape(p["positions"]) == (1, 3) and np.all((np.array(p["positions"]) >= 0) & (np.array(p["positions"]) < 1))
        assert 1.0 <= p["intensity"] < 3.0
        p = corrupt.draw_parameters("RandomGhosting", (4, 4, 4), rng)
        assert 4 <= p["num_ghosts"] <= 10 and p["axis"] in (0, 1, 2) and 0.5 <= p["intensity"] < 1.0 and p["restore"] is True
        seen_axes.add(p["axis"])
        seen_ghosts.add(p["num_ghosts"])
        p = corrupt.draw_parameters("RandomMotion", (4, 4, 4), rng)
        assert np.shape(p["degrees"]) == (2, 3) and np.abs(p["degrees"]).max() <= 30 and np.abs(p["translations"]).max() <= 10
        t = p["times"]
        assert len(t) == 2 and t[0] <= t[1] and all(abs(t[j] - (j + 1) / 3) <= 0.1 + 1e-12 for j in range(2))
    assert seen_axes == {0, 1, 2} and seen_ghosts == set(range(4, 11))
    with pytest.raises(ValueError):
        corrupt.draw_parameters("RandomBlur", (4, 4, 4), np.random.default_rng(0))


# ------------------------------------------------------------------------------------------------ dataset wrapper
class Stub:
    formalized_label_dict = {0: "BG", 1: "LV"}

    def __init__(self, n=2, shape=(3, 8, 6)):
        self.patient_number, self.shape, self._cur = n, shape, None

    def get_patient_data_for_testing(self, i, crop_size=None):
        self._cur = i
        rng = np.random.default_rng(i)
        return {"image": torch.from_numpy(rng.uniform(0, 1, (self.shape[0], 1) + self.shape[1:]).astype(np.float32)),
                "label": torch.from_numpy(rng.integers(0, 2, self.shape))}

    def get_id(self):
        return "patient%03d" % self._cur


def test_corrupted_dataset_ids_counts_and_draws():
    base = Stub()
    for kind in corrupt.KINDS:
        ds = corrupt.CorruptedDataset(base, kind, n_augmented=3, seed=11, host=True)
        assert ds.patient_number == len(ds) == 6 and ds.formalized_label_dict == base.formalized_label_dict
        assert not hasattr(ds, "get_voxel_spacing")                             # optional: offered only when the dataset offers it
        ids, packs = [], []
        for idx in range(6):
            pack = ds.get_patient_data_for_testing(idx, crop_size=None)
            ids.append(ds.get_id())
            packs.append(pack)
            clean = base.get_patient_data_for_testing(idx % 2)
            assert torch.equal(pack["label"], clean["label"])                   # labels are untouched
            assert tuple(pack["image"].shape) == (3, 1, 8, 6) and pack["image"].dtype == torch.float32
            assert float(pack["image"].min()) == 0.0 and float(pack["image"].max()) == 1.0          # rescaled per slice
            assert not torch.equal(pack["image"], clean["image"])
            want = corrupt.corrupt_volume_host(clean["image"].numpy(), kind, ds.parameters(idx, (3, 8, 6)))
            assert np.array_equal(pack["image"].numpy(), want)
        assert ids == ["patient000_0", "patient001_0", "patient000_1", "patient001_1", "patient000_2", "patient001_2"]
        assert not torch.equal(packs[0]["image"], packs[2]["image"])            # another copy, another draw
        again = corrupt.CorruptedDataset(base, kind, n_augmented=3, seed=11, host=True).get_patient_data_for_testing(4)
        assert torch.equal(again["image"], packs[4]["image"])                   # any patient on its own, the same bits
        with pytest.raises(IndexError):
            ds.get_patient_data_for_testing(6)
    base.get_voxel_spacing = lambda: [10.0, 1.25, 1.25]
    assert corrupt.CorruptedDataset(base, "RandomBias").get_voxel_spacing() == [10.0, 1.25, 1.25]
    with pytest.raises(ValueError):
        corrupt.CorruptedDataset(base, "RandomBlur")
