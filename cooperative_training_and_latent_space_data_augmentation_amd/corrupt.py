"""MR artefact corruption of test volumes on the device: the ACDC-C sets of the robustness evaluation.

Mirror of medseg/dataset_loader/generate_artefacted_data.py:56-83, which corrupts every test patient offline with TorchIO
(`RandomBiasField`, `RandomSpike`, `RandomGhosting`, `RandomMotion`: three copies each, rescaled to [0, 1]) and which
medseg/test_ACDC_triplet_segmentation.py:123-124 then scores as `RandomBias`, `RandomSpike`, `RandomGhosting` and `RandomMotion`.
Here a clean device volume [D,H,W] (axes 0, 1, 2: TorchIO's axis order when upstream feeds it CNHW) is corrupted in place of the files:
the host draws the handful of random parameters from a numpy Generator, the kernels of csrc/ctl_corrupt.hip take them as arguments.
None of the four needs an FFT on the device: a spike is a plane wave in image space, and a spectrum mask that varies along one axis
only (ghosting, motion) is a real L x L matrix along that axis, which the host builds in fp64 and the device applies.

The `*_host` functions are the definition: TorchIO's documented arithmetic restated in fp64 numpy (TorchIO and SimpleITK are not
available to check against; DESIGN.md lists what follows from that).  They are what the device results are tested against, and
tests/test_corrupt_host_cpu.py pins them to the literal `fftshift(fftn)` -> edit -> `ifftn` -> real forms."""
import numpy as np
import torch

from . import ops

F32 = np.float32
KINDS = ("RandomBias", "RandomSpike", "RandomGhosting", "RandomMotion")
BIAS_ORDER = 3
BIAS_POWERS = [(i, j, k) for i in range(BIAS_ORDER + 1) for j in range(BIAS_ORDER + 1 - i) for k in range(BIAS_ORDER + 1 - i - j)]


def _volume_host(x):
    x = np.asarray(x)
    if x.ndim == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.ndim != 3 or x.size == 0:
        raise ValueError(f"expected a non-empty [D,H,W] volume (or a [D,1,H,W] pack), got {x.shape}")
    return x.astype(np.float64)


# ------------------------------------------------------------------------------------------------ bias field
def bias_coordinates(n):
    """TorchIO's `arange(-h, h) + 0.5` mesh divided by its maximum, h = n // 2, continued to every index of an odd axis; 0 where h == 0."""
    h = n // 2
    return np.zeros(n) if h == 0 else (np.arange(n, dtype=np.float64) - h + 0.5) / (h - 0.5)


def bias_field_host(x, coefficients):
    """x * exp(sum c_ijk u^i v^j w^k), i + j + k <= 3 in the loop order i, j, k; the coefficients are the float32 values the kernel takes."""
    x = _volume_host(x)
    c = np.asarray(coefficients, dtype=F32).astype(np.float64).reshape(-1)
    assert c.size == len(BIAS_POWERS)
    u, v, w = (bias_coordinates(n) for n in x.shape)
    p = np.zeros(x.shape)
    for cc, (i, j, k) in zip(c, BIAS_POWERS):
        p += cc * (u[:, None, None] ** i) * (v[None, :, None] ** j) * (w[None, None, :] ** k)
    return x * np.exp(p)


# ------------------------------------------------------------------------------------------------ spike
def spike_wave_vectors(shape, positions):
    """The spectrum entries a list of spike positions (fractions of the shape, [n,3]) sets: TorchIO writes the shifted-spectrum indices
    mid + d and mid - d with mid + d = floor(position * shape), i.e. the frequencies d and -d, taken modulo the shape.
    -> (k int32 [m,3], mult int32 [m]): every pair {k, -k} once (the lexicographically smaller member), mult 1 where k == -k."""
    shape = np.asarray(shape, dtype=np.int64)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    index = np.clip(np.floor(pos * shape).astype(np.int64), 0, shape - 1)
    seen, ks, mult = set(), [], []
    for idx in index:
        k = tuple(int(v) for v in (idx - shape // 2) % shape)
        kn = tuple(int(v) for v in (-np.array(k)) % shape)
        key = min(k, kn)
        if key in seen:
            continue
        seen.add(key)
        ks.append(key)
        mult.append(1 if k == kn else 2)
    return np.array(ks, dtype=np.int32).reshape(-1, 3), np.array(mult, dtype=np.int32)


def _plane_wave(shape, k):
    """exp(+2 pi i k.r / shape) on the grid, the phase reduced exactly in integers per axis"""
    e = [np.exp(2j * np.pi * ((int(k[a]) * np.arange(n, dtype=np.int64)) % n) / n) for a, n in enumerate(shape)]
    return e[0][:, None, None] * e[1][None, :, None] * e[2][None, None, :]


def spike_host(x, positions, intensity):
    """RandomSpike in image space: out = x + (1/N) Re sum_{q in {k, -k}} (A - X[q]) exp(+2 pi i q.r / shape), A = intensity * sum(x), every
    spike applied to the same original spectrum.  Defined for non-negative volumes (sum(x) is then the peak numpy's complex max finds)."""
    x = _volume_host(x)
    assert x.min() >= 0, "spike: defined for non-negative volumes (A = intensity * sum(x) is the peak of the spectrum only then)"
    ks, mult = spike_wave_vectors(x.shape, positions)
    amp = float(intensity) * x.sum()
    out = x.copy()
    for k, m in zip(ks, mult):
        wave = _plane_wave(x.shape, k)
        xk = (x * np.conj(wave)).sum()
        out += m * ((amp - xk) * wave).real / x.size
    return out


# ------------------------------------------------------------------------------------------------ operators along one axis
def mask_operator(mask):
    """Re(F^-1 diag(ifftshift(mask)) F) for a real mask over the SHIFTED spectrum of an axis of len(mask) elements: fp64 [L, L]"""
    m = np.fft.ifftshift(np.asarray(mask, dtype=np.float64))
    return np.fft.ifft(m[:, None] * np.fft.fft(np.eye(m.size), axis=0), axis=0).real


def apply_operator_host(volumes, matrix, axis):
    """out[r, j] = sum_t sum_k matrix[j, t L + k] volumes[t][r, k] along `axis`, fp64"""
    length = volumes[0].shape[axis]
    out = np.zeros(volumes[0].shape)
    for t, v in enumerate(volumes):
        c = np.asarray(matrix, dtype=np.float64)[:, t * length:(t + 1) * length]
        out += np.moveaxis(np.tensordot(c, np.asarray(v, dtype=np.float64), axes=([1], [axis])), 0, axis)
    return out


def ghosting_mask(length, num_ghosts, intensity, restore=True):
    """1 - intensity on the planes 0, n, 2n, ... of the shifted spectrum, the plane length // 2 put back with `restore`"""
    m = np.ones(length)
    m[::int(num_ghosts)] = 1.0 - float(intensity)
    if restore:
        m[length // 2] = 1.0
    return m


def ghosting_operator(length, num_ghosts, intensity, restore=True):
    return mask_operator(ghosting_mask(length, num_ghosts, intensity, restore))


def ghosting_host(x, num_ghosts, axis, intensity, restore=True):
    x = _volume_host(x)
    return apply_operator_host([x], ghosting_operator(x.shape[axis], num_ghosts, intensity, restore), axis)


# ------------------------------------------------------------------------------------------------ motion
def rigid_matrices(shape, spacing, degrees, translations):
    """[T,3,4] fp64 voxel-space maps p -> source voxel: the output point in millimetres (spacing * p) is rotated about the volume's
    physical centre c = spacing * (shape - 1) / 2 by R = Rz Rx Ry (SimpleITK's default Euler order; axes 0, 1, 2 are x, y, z), translated,
    and divided by the spacing: M[a][b] = R[a][b] spacing[b] / spacing[a], o = (c - R c + t) / spacing.  Zero angles and translations give
    the identity exactly."""
    s = np.ones(3) if spacing is None else np.asarray(spacing, dtype=np.float64).reshape(3)
    if not np.all(s > 0):
        raise ValueError("motion: spacings must be positive")
    deg = np.asarray(degrees, dtype=np.float64).reshape(-1, 3)
    tr = np.asarray(translations, dtype=np.float64).reshape(-1, 3)
    if deg.shape != tr.shape:
        raise ValueError("motion: one translation per rotation")
    c = s * (np.asarray(shape, dtype=np.float64) - 1) / 2
    out = np.zeros((deg.shape[0], 3, 4))
    for t in range(deg.shape[0]):
        ax, ay, az = np.radians(deg[t])
        cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        r = rz @ rx @ ry
        out[t, :, :3] = r * s[None, :] / s[:, None]
        out[t, :, 3] = (c - r @ c + tr[t]) / s
    return out


def rigid3d_host(x, matrices):
    """[T,D,H,W] fp64: the volume, extended by zeros, interpolated linearly at M p + o, with the float32 matrix values the kernel takes"""
    x = _volume_host(x)
    m = np.asarray(matrices, dtype=F32).astype(np.float64).reshape(-1, 3, 4)
    pad = np.pad(x, 1)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in x.shape], indexing="ij"))
    out = np.zeros((m.shape[0],) + x.shape)
    for t in range(m.shape[0]):
        src = np.tensordot(m[t, :, :3], grid, axes=([1], [0])) + m[t, :, 3][:, None, None, None]
        inside = np.ones(x.shape, dtype=bool)
        for a, n in enumerate(x.shape):
            inside &= (src[a] > -1) & (src[a] < n)
        lo = [np.clip(np.floor(src[a]), -1, n - 1) for a, n in enumerate(x.shape)]
        f = [src[a] - lo[a] for a in range(3)]
        i0 = [l.astype(np.int64) + 1 for l in lo]                        # indices into the padded volume
        acc = np.zeros(x.shape)
        for da in (0, 1):
            for db in (0, 1):
                for dc in (0, 1):
                    wgt = (f[0] if da else 1 - f[0]) * (f[1] if db else 1 - f[1]) * (f[2] if dc else 1 - f[2])
                    acc += wgt * pad[i0[0] + da, i0[1] + db, i0[2] + dc]
        out[t] = np.where(inside, acc, 0.0)
    return out


def motion_segments(length, times):
    """Which volume fills which part of the shifted spectrum of the last axis: [T + 1, L] masks for the volumes [x, copy_1, ..., copy_T].
    The segments [0, i_0), [i_0, i_1), ..., [i_{T-1}, L) with i = floor(L * times) belong to the volumes in that order, after the swap
    that gives the segment containing L // 2 to the unmoved x and segment 0 to the volume it displaces."""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    if np.any(np.diff(times) < 0) or np.any(times < 0) or np.any(times > 1):
        raise ValueError("motion: times must be sorted and inside [0, 1]")
    edges = [0] + [int(v) for v in np.floor(length * times)] + [length]
    centre = next(i for i in range(len(edges) - 1) if edges[i] <= length // 2 < edges[i + 1])
    owner = list(range(len(edges) - 1))                                  # owner[segment] = volume
    owner[0], owner[centre] = owner[centre], owner[0]
    masks = np.zeros((len(edges) - 1, length))
    for seg, vol in enumerate(owner):
        masks[vol, edges[seg]:edges[seg + 1]] = 1.0
    return masks


def motion_operator(length, times):
    """[L, (T + 1) L] fp64: the operators of the T + 1 segment masks side by side"""
    return np.concatenate([mask_operator(m) for m in motion_segments(length, times)], axis=1)


def motion_host(x, spacing, degrees, translations, times):
    x = _volume_host(x)
    copies = rigid3d_host(x, rigid_matrices(x.shape, spacing, degrees, translations))
    return apply_operator_host([x] + list(copies), motion_operator(x.shape[2], times), 2)


# ------------------------------------------------------------------------------------------------ parameters
def draw_parameters(kind, shape, rng):
    """The random parameters of one corruption as a plain dict, drawn as TorchIO's defaults in generate_artefacted_data.py draw them:
    RandomBias coefficients ~ U(-0.5, 0.5); RandomSpike one position ~ U(0, 1)^3, intensity ~ U(1, 3); RandomGhosting num_ghosts in
    4..10, axis in {0, 1, 2}, intensity ~ U(0.5, 1); RandomMotion (degrees=30, translation=10, two transforms) degrees ~ U(-30, 30)^3,
    translations ~ U(-10, 10)^3 mm, times (j + 1) / (T + 1) + U(-0.3, 0.3) / (T + 1), sorted."""
    if kind == "RandomBias":
        return {"coefficients": [float(v) for v in rng.uniform(-0.5, 0.5, len(BIAS_POWERS))]}
    if kind == "RandomSpike":
        return {"positions": rng.uniform(0.0, 1.0, (1, 3)).tolist(), "intensity": float(rng.uniform(1.0, 3.0))}
    if kind == "RandomGhosting":
        return {"num_ghosts": int(rng.integers(4, 11)), "axis": int(rng.integers(0, 3)), "intensity": float(rng.uniform(0.5, 1.0)),
                "restore": True}
    if kind == "RandomMotion":
        t = 2
        degrees, translations = rng.uniform(-30.0, 30.0, (t, 3)), rng.uniform(-10.0, 10.0, (t, 3))
        times = np.sort((np.arange(t) + 1.0) / (t + 1) + rng.uniform(-0.3, 0.3, t) / (t + 1))
        return {"degrees": degrees.tolist(), "translations": translations.tolist(), "times": times.tolist()}
    raise ValueError(f"kind {kind!r}: one of {KINDS}")


# ------------------------------------------------------------------------------------------------ device path
class Corruption:
    """One corruption with fixed parameters for volumes of one shape: everything the kernels read besides the volume (operator matrix,
    workspace, the stack of rigid copies) is made here, so a call only enqueues kernels and can be captured in a graph."""

    def __init__(self, kind, params, shape, spacing=None, device=None):
        if kind not in KINDS:
            raise ValueError(f"kind {kind!r}: one of {KINDS}")
        shape = tuple(int(v) for v in shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"expected a [D,H,W] shape, got {shape}")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.kind, self.params, self.shape = kind, dict(params), shape
        p = self.params
        if kind == "RandomBias":
            self.coefficients = np.asarray(p["coefficients"], dtype=F32)
        elif kind == "RandomSpike":
            self.k, self.mult = spike_wave_vectors(shape, p["positions"])
            self.workspace = ops.corrupt_spike_workspace(shape, len(self.mult), dev)
        elif kind == "RandomGhosting":
            self.axis = int(p["axis"])
            c = ghosting_operator(shape[self.axis], p["num_ghosts"], p["intensity"], p.get("restore", True))
            self.operator = torch.from_numpy(c.astype(F32)).to(dev)
        else:
            self.matrices = rigid_matrices(shape, spacing, p["degrees"], p["translations"]).astype(F32)
            self.operator = torch.from_numpy(motion_operator(shape[2], p["times"]).astype(F32)).to(dev)
            if self.operator.shape[1] != (len(self.matrices) + 1) * shape[2]:
                raise ValueError("motion: one time per transform")
            self.stack = torch.empty((len(self.matrices),) + shape, dtype=torch.float32, device=dev)

    def __call__(self, x, out=None):
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if tuple(x.shape) != self.shape:
            raise ValueError(f"{self.kind}: made for volumes {self.shape}, got {tuple(x.shape)}")
        if self.kind == "RandomBias":
            return ops.corrupt_bias_field(x, self.coefficients, out=out)
        if self.kind == "RandomSpike":
            return ops.corrupt_spike(x, self.k, self.mult, self.params["intensity"], out=out, workspace=self.workspace)
        if self.kind == "RandomGhosting":
            return ops.axis_operator(x, self.operator, self.axis, out=out)
        ops.corrupt_rigid3d(x, self.matrices, out=self.stack)
        return ops.axis_operator(x, self.operator, 2, stack=self.stack, out=out)


def bias_field(x, coefficients, out=None):
    """RandomBiasField(coefficients=0.5, order=3) with given coefficients: x [D,H,W] float32 on the device -> the same.  One launch."""
    return Corruption("RandomBias", {"coefficients": coefficients}, _shape3(x))(x, out)


def _shape3(x):
    return tuple(x.shape) if x.dim() == 3 else (int(x.shape[0]),) + tuple(x.shape[2:])


def spike(x, positions, intensity, out=None):
    """RandomSpike with given positions ([n,3] fractions of the shape) and intensity, for a non-negative volume.  Two launches."""
    return Corruption("RandomSpike", {"positions": positions, "intensity": intensity}, _shape3(x))(x, out)


def ghosting(x, num_ghosts, axis, intensity, restore=True, out=None):
    """RandomGhosting with given parameters: the host builds the operator of the axis in fp64, the device applies it.  One launch."""
    return Corruption("RandomGhosting", {"num_ghosts": num_ghosts, "axis": axis, "intensity": intensity, "restore": restore}, _shape3(x))(x, out)


def motion(x, spacing, degrees, translations, times, out=None):
    """RandomMotion with given transforms ([T,3] degrees, [T,3] mm) and times ([T], sorted); spacing None = (1, 1, 1).  Two launches."""
    return Corruption("RandomMotion", {"degrees": degrees, "translations": translations, "times": times}, _shape3(x), spacing=spacing)(x, out)


def _parameters(kind, shape, params_or_seed):
    if isinstance(params_or_seed, dict):
        return params_or_seed
    return draw_parameters(kind, shape, np.random.default_rng(params_or_seed))


def corrupt_volume(x, kind, params_or_seed, spacing=None, rescale=True):
    """One ACDC-C copy of a device volume: x [D,H,W] or a tester pack [D,1,H,W] (float32, non-negative for RandomSpike) -> the same shape.
    params_or_seed: the dict of draw_parameters, or a seed for it.  rescale: every slice to [0, 1] with ops.rescale_intensity, as
    generate_artefacted_data.py:82 does."""
    shape = _shape3(x)
    out = Corruption(kind, _parameters(kind, shape, params_or_seed), shape, spacing=spacing)(x)
    out = out.unsqueeze(1)
    if rescale:
        out = ops.rescale_intensity(out, 0.0, 1.0)
    return out if x.dim() == 4 else out[:, 0]


def corrupt_volume_host(x, kind, params_or_seed, spacing=None, rescale=True):
    """corrupt_volume as the fp64 host statements, returned as float32 (the per-slice rescale in fp64, eps 1e-20 as the device's)."""
    v = _volume_host(x)
    p = _parameters(kind, v.shape, params_or_seed)
    if kind == "RandomBias":
        out = bias_field_host(v, p["coefficients"])
    elif kind == "RandomSpike":
        out = spike_host(v, p["positions"], p["intensity"])
    elif kind == "RandomGhosting":
        out = ghosting_host(v, p["num_ghosts"], p["axis"], p["intensity"], p.get("restore", True))
    elif kind == "RandomMotion":
        out = motion_host(v, spacing, p["degrees"], p["translations"], p["times"])
    else:
        raise ValueError(f"kind {kind!r}: one of {KINDS}")
    if rescale:
        mn, mx = out.min(axis=(1, 2), keepdims=True), out.max(axis=(1, 2), keepdims=True)
        out = (out - mn) / ((mx - mn) + 1e-20)
    out = out.astype(F32)
    return out[:, None] if np.ndim(x) == 4 else out


class CorruptedDataset:
    """`n_augmented` corrupted copies of every patient of a test dataset, what generate_artefacted_data.py writes to disk: patient
    j * patient_number + i is copy j of patient i (upstream's loop order), its id is "{pid}_{j}", its label is the clean one.  The wrapped
    dataset offers `patient_number`, `get_patient_data_for_testing(i, crop_size=)` and `get_id()`; everything else (`get_voxel_spacing`,
    `formalized_label_dict`, ...) is passed through when it is there.  The parameters of copy (i, j) are drawn from
    numpy.random.default_rng([seed, j, i]), so any patient can be made on its own.  host=True: the fp64 host statements instead."""

    def __init__(self, test_dataset, kind, n_augmented=3, seed=0, host=False):
        if kind not in KINDS:
            raise ValueError(f"kind {kind!r}: one of {KINDS}")
        self.test_dataset, self.kind, self.n_augmented, self.seed, self.host = test_dataset, kind, int(n_augmented), int(seed), bool(host)
        self.patient_number = test_dataset.patient_number * self.n_augmented
        self.last_params, self._copy = None, None

    def __len__(self):
        return self.patient_number

    def __getattr__(self, name):                                           # only reached for what this class does not define
        if name == "test_dataset":
            raise AttributeError(name)
        return getattr(self.test_dataset, name)

    def parameters(self, index, shape):
        j, i = divmod(int(index), self.test_dataset.patient_number)
        return draw_parameters(self.kind, shape, np.random.default_rng([self.seed, j, i]))

    def get_patient_data_for_testing(self, index, crop_size=None):
        if not 0 <= index < self.patient_number:
            raise IndexError(index)
        j, i = divmod(int(index), self.test_dataset.patient_number)
        pack = dict(self.test_dataset.get_patient_data_for_testing(i, crop_size=crop_size))
        image = torch.as_tensor(pack["image"])
        if image.dim() == 5:
            image = image[0]
        self._copy = j
        self.last_params = self.parameters(index, (int(image.shape[0]),) + tuple(int(v) for v in image.shape[-2:]))
        if self.host:
            pack["image"] = torch.from_numpy(corrupt_volume_host(image.float().cpu().numpy(), self.kind, self.last_params))
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
            pack["image"] = corrupt_volume(image.to(dev, dtype=torch.float32), self.kind, self.last_params)
        return pack

    def get_id(self):
        return "{}_{}".format(self.test_dataset.get_id(), self._copy)
