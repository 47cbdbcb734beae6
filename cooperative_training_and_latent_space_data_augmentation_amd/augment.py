"""Training augmentation of a batch on the device (medseg/dataset_loader/transform.py:46-86, which upstream runs per slice on the host
inside DataLoader workers): flip, contrast / brightness, random affine, choice rotation, elastic deformation, centre crop, min-max
normalisation.  The parameters of every sample are drawn on the host (a few floats); the pixels never leave the device, and image and
label are resampled once.  The semantics are written out in include/ctl_hip.h next to ctl_aug_field / ctl_aug_warp; `apply_host` states
them again in fp64 numpy / scipy and is the host path for numpy inputs.

    aug = BatchAugmenter("ACDC_affine_elastic_intensity", crop_size=(192, 192), seed=0)
    image, label = aug(image, label)          # [n,1,Hp,Wp] float32, [n,Hp,Wp] int64 on the device -> [n,1,192,192], [n,192,192]

BatchAugmenter(..., interp="cubic", num_classes=K) reads image and label through upstream's cubic spline (ctl_aug_warp_cubic) in place of
bilinear / nearest; the default is unchanged.

BatchAugmenter.from_config(config, crop_size) takes upstream's config dict (the keys of transform.py:114-144) in place of a policy name
and adds the bias field of MyRandomPurtarbationV2 (ctl_aug_bias) and the coarse-grid elastic deformation of MyElasticTransformCoarseGrid
(ctl_aug_coarse_field); reference_config(name) is upstream's dict for each of its 24 names.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

CONTRAST_RANGE = (0.8, 1.2)          # RandomBrightnessFluctuation defaults, _utils/intensity_transform.py:120
BRIGHTNESS_RANGE = (-0.1, 0.1)
ALPHA_RANGE = (1.5, 2.0)             # alpha = Hp * U(1.5, 2), sigma = Hp * U(0.1, 0.2) * 3 / 4: _utils/elastic_transform.py:72-75
SIGMA_RANGE = (0.1, 0.2)
SIGMA_FACTOR = 0.75


def _policy(flip=(False, False, 0.0), shift=(0.0, 0.0), rotate=0.0, scale=(1.0, 1.0), shear=0.0, rotate_groups=(), intensity_prob=0.0,
            elastic_prob=0.0):
    return {"flip": tuple(flip), "shift": tuple(shift), "rotate": float(rotate), "scale": tuple(scale), "shear": float(shear),
            "rotate_groups": tuple(rotate_groups), "intensity_prob": float(intensity_prob), "elastic_prob": float(elastic_prob)}


_AFFINE = dict(shift=(0.1, 0.1), rotate=15, scale=(0.9, 1.1))
_ACDC = dict(flip=(True, True, 0.2), shift=(0.1, 0.1), rotate=15, scale=(0.8, 1.1), rotate_groups=tuple(45 * i for i in range(8)))
# the ranges of transform.py:114-313 for the policies the supported transforms can express
POLICIES = {
    "no_aug": _policy(),
    "affine": _policy(**_AFFINE),
    "scale": _policy(scale=(0.8, 1.2)),
    "elastic": _policy(elastic_prob=1.0),
    "elastic_scale": _policy(scale=(0.9, 1.1), elastic_prob=0.5),
    "affine_elastic": _policy(elastic_prob=0.5, **_AFFINE),
    "ACDC_affine": _policy(**_ACDC),
    "ACDC_affine_intensity": _policy(intensity_prob=0.5, **_ACDC),
    "ACDC_affine_elastic": _policy(elastic_prob=0.5, **_ACDC),
    "ACDC_affine_elastic_intensity": _policy(intensity_prob=0.5, elastic_prob=0.5, **_ACDC),
    "Prostate_affine_elastic_intensity": _policy(flip=(True, True, 0.5), shift=(0.1, 0.1), rotate=15, scale=(0.8, 1.2), intensity_prob=0.5,
                                                 elastic_prob=0.5),
}
# the other names of transform.py:16-41 and the transform each needs that is not built here
UNSUPPORTED = {
    "gamma": "RandomGamma", "gamma_scale": "RandomGamma", "gamma_elastic": "RandomGamma", "affine_gamma": "RandomGamma",
    "affine_gamma_elastic": "RandomGamma", "Atrial_basic": "RandomGamma", "Atrial_perturb": "RandomGamma and MyRandomPurtarbation",
    "ACDC_affine_perturb": "MyRandomPurtarbation", "ACDC_affine_perturb_v2": "MyRandomPurtarbationV2",
    "ACDC_affine_elastic_bias": "MyRandomPurtarbationV2", "ACDC_affine_all": "MyRandomPurtarbationV2",
    "ACDC_affine_elastic_intensity_v2": "MyElasticTransformCoarseGrid", "elastic_v2": "MyElasticTransformCoarseGrid",
}


def get_policy(name: str) -> dict:
    if name in POLICIES:
        return POLICIES[name]
    if name in UNSUPPORTED:
        raise NotImplementedError(f"data_aug_policy {name!r} needs {UNSUPPORTED[name]}, which is not implemented on the device "
                                  f"(supported: {', '.join(POLICIES)})")
    raise KeyError(f"unknown data_aug_policy {name!r}")


# ---------------------------------------------------------------------------------------------- config dicts
def no_aug_config() -> dict:
    """The keys and defaults of upstream's no_aug() (transform.py:114-144)."""
    return {"flip_flag": [False, False, 0.0], "shift_val": (0.0, 0.0), "rotate_val": 0, "scale_val": (1.0, 1.0), "rotate_groups": [],
            "intensity_prob": 0, "gamma_prob": 0.0, "gamma_range": [0.8, 1.2], "elastic_prob": 0.0, "shear_val": 0, "elastic_probv2": 0,
            "perturb_prob": 0.0, "max_sigma": 16, "multi_control_points": [4], "add_noise": False, "noise_epsilon": 0.01,
            "perturb_v2_prob": 0.0, "perturb_v2_bias_magnitude": 0.2, "ms_control_point_spacing": [32], "perturb_v2_add_noise": False,
            "perturb_v2_noise_epsilon": 0.01}


_C_AFFINE = {"shift_val": (0.1, 0.1), "rotate_val": 15, "scale_val": (0.9, 1.1)}
_C_ACDC = {"flip_flag": [True, True, 0.2], "shift_val": (0.1, 0.1), "rotate_val": 15, "scale_val": (0.8, 1.1),
           "rotate_groups": [45 * i for i in range(8)]}
_C_ATRIAL = {"flip_flag": [True, True, 0.5], "shift_val": (0.1, 0.1), "rotate_val": 10, "scale_val": (0.7, 1.3), "gamma_range": (0.8, 2.0),
             "gamma_prob": 0.5}
_C_GAMMA = {"gamma_prob": 0.5, "gamma_range": [0.8, 1.2]}
_C_V1 = {"perturb_prob": 0.5, "max_sigma": 16, "multi_control_points": [2, 4, 8]}
_C_V2 = {"perturb_v2_prob": 0.5, "perturb_v2_bias_magnitude": 0.3, "ms_control_point_spacing": [64, 1], "perturb_v2_add_noise": True,
         "perturb_v2_noise_epsilon": 0.01}
# what each name of transform.py:16-41 writes over no_aug(), with the numbers of transform.py:146-313.  'affine_gamma' is mapped to the
# affine-elastic config there (:26), and ACDC_affine_perturb writes a key 'epsilon' that nothing reads (:228); both are kept.
_REFERENCE_CONFIGS = {
    "no_aug": {},
    "gamma": _C_GAMMA,
    "gamma_scale": {**_C_GAMMA, "scale_val": [0.9, 1.1]},
    "affine": _C_AFFINE,
    "scale": {"scale_val": (0.8, 1.2)},
    "elastic": {"elastic_prob": 1},
    "elastic_scale": {"elastic_prob": 0.5, "scale_val": [0.9, 1.1]},
    "gamma_elastic": {**_C_GAMMA, "elastic_prob": 0.5},
    "affine_elastic": {**_C_AFFINE, "elastic_prob": 0.5},
    "affine_gamma": {**_C_AFFINE, "elastic_prob": 0.5},
    "affine_gamma_elastic": {**_C_AFFINE, **_C_GAMMA, "elastic_prob": 0.5},
    "ACDC_affine": _C_ACDC,
    "ACDC_affine_perturb": {**_C_ACDC, **_C_V1, "add_noise": True, "epsilon": 0.01},
    "ACDC_affine_perturb_v2": {**_C_ACDC, **_C_V2},
    "ACDC_affine_elastic": {**_C_ACDC, "elastic_prob": 0.5},
    "ACDC_affine_intensity": {**_C_ACDC, "intensity_prob": 0.5},
    "ACDC_affine_elastic_intensity": {**_C_ACDC, "intensity_prob": 0.5, "elastic_prob": 0.5},
    "ACDC_affine_elastic_intensity_v2": {**_C_ACDC, "intensity_prob": 0.5, "elastic_probv2": 0.5},
    "ACDC_affine_elastic_bias": {**_C_ACDC, **_C_V2, "elastic_prob": 0.5},
    "ACDC_affine_all": {**_C_ACDC, **_C_V2, "elastic_prob": 0.5, "intensity_prob": 0.5},
    "Atrial_basic": _C_ATRIAL,
    "Atrial_perturb": {**_C_ATRIAL, **_C_V1},
    "Prostate_affine_elastic_intensity": {"flip_flag": [True, True, 0.5], "shift_val": (0.1, 0.1), "rotate_val": 15, "scale_val": (0.8, 1.2),
                                          "intensity_prob": 0.5, "elastic_prob": 0.5},
    "elastic_v2": {"elastic_probv2": 1},
}
IGNORED_CONFIG_KEYS = ("gamma_prob", "gamma_range", "ms_control_point_spacing")


def reference_config(name: str) -> dict:
    """Upstream's config dict for one of its 24 policy names (a fresh copy).  A table of settings: whether BatchAugmenter(name) runs is
    still decided by POLICIES / UNSUPPORTED."""
    if name not in _REFERENCE_CONFIGS:
        raise KeyError(f"unknown data_aug_policy {name!r}")
    config = no_aug_config()
    for k, v in _REFERENCE_CONFIGS[name].items():
        config[k] = list(v) if isinstance(v, list) else v
    return config


def policy_from_config(config: dict) -> dict:
    """The policy dict BatchAugmenter draws from (the form of POLICIES, plus coarse_prob, bias_prob, bias_m, bias_eps) for an upstream
    config dict.  Missing keys take no_aug()'s values."""
    if float(config.get("perturb_prob", 0.0)) > 0.0:
        raise NotImplementedError("config['perturb_prob'] > 0 asks for MyRandomPurtarbation (V1), which is not implemented: upstream resizes "
                                  "its float32 field through Image.fromarray(..., mode='L') (intensity_transform.py:339-341), which reads "
                                  "the raw float bytes as 8-bit pixels, so there is no well-defined field to reproduce")
    cfg = no_aug_config()
    unknown = sorted(set(config) - set(cfg))
    if unknown:
        raise KeyError(f"unknown config key(s) {unknown}; the keys are those of no_aug() (transform.py:114-144): {sorted(cfg)}")
    cfg.update(config)
    if float(cfg["elastic_prob"]) > 0.0 and float(cfg["elastic_probv2"]) > 0.0:
        raise ValueError("config sets both elastic_prob and elastic_probv2: two successive warps are not one displacement field")
    m = float(cfg["perturb_v2_bias_magnitude"])
    if float(cfg["perturb_v2_prob"]) > 0.0 and not abs(m) < 1.0:
        raise ValueError(f"perturb_v2_bias_magnitude must be below 1 in magnitude (intensity_transform.py:402), got {m}")
    p = _policy(flip=cfg["flip_flag"], shift=cfg["shift_val"], rotate=cfg["rotate_val"], scale=cfg["scale_val"], shear=cfg["shear_val"],
                rotate_groups=cfg["rotate_groups"], intensity_prob=cfg["intensity_prob"], elastic_prob=cfg["elastic_prob"])
    p.update(coarse_prob=float(cfg["elastic_probv2"]), bias_prob=float(cfg["perturb_v2_prob"]), bias_m=abs(m),
             bias_eps=float(cfg["perturb_v2_noise_epsilon"]) if cfg["perturb_v2_add_noise"] else 0.0)
    return p


def crop_offsets(hp: int, wp: int, hc: int, wc: int):
    """First row / column of the centre window: ceil((Hp - Hc) / 2) (MySpecialCrop, _utils/affine_transform.py:280-283)."""
    return (hp - hc + 1) // 2, (wp - wc + 1) // 2


def _cos_sin_deg(deg):
    """cos / sin of angles in degrees, exact at the multiples of 90 so that quarter turns map pixel centres onto pixel centres."""
    deg = np.asarray(deg, dtype=np.float64)
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    quarter = np.mod(deg, 90.0) == 0
    k = np.mod(np.round(deg / 90.0), 4).astype(np.int64)
    c = np.where(quarter, np.array([1.0, 0.0, -1.0, 0.0])[k], c)
    s = np.where(quarter, np.array([0.0, 1.0, 0.0, -1.0])[k], s)
    return c, s


def _rot(deg):
    c, s = _cos_sin_deg(deg)
    m = np.zeros(c.shape + (3, 3))
    m[..., 0, 0], m[..., 0, 1], m[..., 1, 0], m[..., 1, 1], m[..., 2, 2] = c, -s, s, c, 1.0
    return m


def compose_matrix(flip, theta, translate, zoom, choice, hp: int, wp: int, shear=None) -> np.ndarray:
    """M = F A Rc, A = R(theta) T(ty, tx) Sh(phi) Z(zy, zx): the fp64 [n,2,3] output -> input maps about the plane centre in (row, col)
    order.  flip [n,2] = (horizontal: columns reversed, vertical: rows reversed); theta, choice, shear in degrees; translate [n,2] =
    (fraction of the height, fraction of the width); zoom [n,2] = (rows, cols).  The factor order of A is torchsample's RandomAffine as
    documented (a definition here)."""
    flip = np.asarray(flip, dtype=bool).reshape(-1, 2)
    n = flip.shape[0]
    translate = np.asarray(translate, dtype=np.float64).reshape(n, 2)
    zoom = np.asarray(zoom, dtype=np.float64).reshape(n, 2)
    shear = np.zeros(n) if shear is None else np.asarray(shear, dtype=np.float64).reshape(n)
    eye = np.broadcast_to(np.eye(3), (n, 3, 3))
    f = eye.copy()
    f[:, 0, 0] = np.where(flip[:, 1], -1.0, 1.0)
    f[:, 1, 1] = np.where(flip[:, 0], -1.0, 1.0)
    t = eye.copy()
    t[:, 0, 2], t[:, 1, 2] = translate[:, 0] * hp, translate[:, 1] * wp
    sh = eye.copy()
    sc, ss = _cos_sin_deg(shear)
    sh[:, 0, 1], sh[:, 1, 1] = -ss, sc
    z = eye.copy()
    z[:, 0, 0], z[:, 1, 1] = zoom[:, 0], zoom[:, 1]
    m = f @ _rot(np.asarray(theta, dtype=np.float64).reshape(n)) @ t @ sh @ z @ _rot(np.asarray(choice, dtype=np.float64).reshape(n))
    return np.ascontiguousarray(m[:, :2, :])


# ---------------------------------------------------------------------------------------------- host statement of the semantics
def _mix(z: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser on uint64 arrays (ctl_mix64 of csrc/ctl_device.h)."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hash_noise(seeds, hp: int, wp: int) -> np.ndarray:
    """u of ctl_aug_field without a noise array: fp64 [n,2,hp,wp], exactly the device's values."""
    seeds = np.asarray(seeds, dtype=np.int64).astype(np.uint64).reshape(-1)
    n = seeds.shape[0]
    plane = np.arange(n * 2, dtype=np.uint64).reshape(n, 2, 1) << np.uint64(32)
    pixel = np.arange(hp * wp, dtype=np.uint64).reshape(1, 1, -1)
    h = _mix(seeds.reshape(n, 1, 1) ^ _mix(plane | pixel))
    return ((h >> np.uint64(40)).astype(np.float64) * 2.0 ** -23 - 1.0).reshape(n, 2, hp, wp)


def elastic_field_host(alpha, sigma, hp: int, wp: int, seeds=None, noise=None) -> np.ndarray:
    """fp64 [n,2,hp,wp]: alpha * scipy.ndimage.gaussian_filter(u, sigma, mode='constant', cval=0, truncate=4.0) per sample and axis."""
    from scipy import ndimage
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    u = hash_noise(seeds, hp, wp) if noise is None else np.asarray(noise, dtype=np.float64)
    out = np.zeros((alpha.shape[0], 2, hp, wp))
    for b in range(alpha.shape[0]):
        if alpha[b] != 0:
            for a in range(2):
                out[b, a] = alpha[b] * ndimage.gaussian_filter(u[b, a], sigma=sigma[b], mode="constant", cval=0.0, truncate=4.0)
    return out


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


# bias field (MyRandomPurtarbationV2, _utils/intensity_transform.py:373-546) -- the record layout is that of ctl_aug_bias in include/ctl_hip.h
BIAS_FLOATS = 192
BIAS_SPACING = 64                    # the V2 constructor overwrites whatever spacing it is given (intensity_transform.py:404)
BIAS_SIDES = (128, 512)
COARSE_FLOATS = 24
COARSE_SIGMA = 10.0                  # MyElasticTransformCoarseGrid(mu=0, sigma=10), elastic_transform.py:107


def bias_grid(hp: int):
    """(h, xmax, x): the extended side, its half and the coarse grid of intensity_transform.py:444-461 for an Hp x Hp plane."""
    h = int(np.round(hp + BIAS_SPACING * 1.5))
    xmax = h // 2
    return h, xmax, np.arange(-xmax, xmax + 1, BIAS_SPACING)


def check_bias_side(hp: int, wp: int) -> None:
    if hp != wp or hp % 2 or not BIAS_SIDES[0] <= hp <= BIAS_SIDES[1]:
        raise ValueError(f"the bias-field stage needs a square plane with an even side of {BIAS_SIDES[0]}..{BIAS_SIDES[1]} (upstream asserts "
                         f"a square plane and at least four control points, intensity_transform.py:439, :448), got {hp}x{wp}")


def _bspline_basis(t, x):
    """FITPACK's fpbspl for degree 3, as ctl_aug_bias evaluates it: x clamped to [t[3], t[-4]]; (h [len(x),4], l [len(x)]) with h[:, i] =
    B_{l+i}(x), the four basis functions that are not zero on the span of x."""
    t = np.asarray(t, dtype=np.float64)
    nt = t.shape[0]
    x = np.clip(np.asarray(x, dtype=np.float64), t[3], t[nt - 4])
    l = np.clip(np.searchsorted(t, x, side="right") - 1, 3, nt - 5)
    h = np.zeros(x.shape + (4,))
    h[:, 0] = 1.0
    for j in range(1, 4):
        hh = h.copy()
        h[:, 0] = 0.0
        for i in range(j):
            li = l + 1 + i
            lj = li - j
            f = hh[:, i] / (t[li] - t[lj])
            h[:, i] += f * (t[li] - x)
            h[:, i + 1] = f * (x - t[lj])
    return h, l - 3


def bias_record(z, hp: int, m: float, eps: float, on: bool = True, tck=None, dtype=np.float32) -> np.ndarray:
    """One sample's record for ctl_aug_bias ([192], see include/ctl_hip.h) from the knot values z [k,k] on bias_grid(hp): the fit
    RectBivariateSpline(x, x, z, s=3, kx=3, ky=3) and the scalar h w / (sum of the spline over arange(-xmax, xmax)^2 + 1e-12), the sum
    taken from separability in fp64: (sum_y B_i(y))^T C (sum_x B_j(x)).  tck = (row knots, column knots, coefficients) replaces the fit.
    dtype float64 keeps the unrounded values (what the host checks against upstream's arithmetic)."""
    rec = np.zeros(BIAS_FLOATS, dtype=np.float64)
    if not on:
        return rec.astype(dtype)
    h, xmax, x = bias_grid(hp)
    if tck is None:
        from scipy.interpolate import RectBivariateSpline
        tck = RectBivariateSpline(x, x, np.asarray(z, dtype=np.float64), s=3, kx=3, ky=3).tck[:3]
    t0, t1, c = (np.asarray(v, dtype=np.float64) for v in tck)
    n0, n1 = t0.shape[0], t1.shape[0]
    if not (8 <= n0 <= 16 and 8 <= n1 <= 16):
        raise ValueError(f"bias_record: {n0} x {n1} knots; the record holds 8..16 per axis")
    c = c.reshape(n0 - 4, n1 - 4)
    grid = np.arange(-xmax, xmax, dtype=np.float64)
    sums = []
    for t in (t0, t1):
        b, l = _bspline_basis(t, grid)
        acc = np.zeros(t.shape[0] - 4)
        for i in range(4):
            np.add.at(acc, l + i, b[:, i])
        sums.append(acc)
    total = sums[0] @ c @ sums[1]
    rec[0], rec[1], rec[2], rec[3], rec[4], rec[5] = 1.0, n0, n1, (h * h) / (total + 1e-12), abs(m), eps
    rec[8:8 + n0], rec[24:24 + n1] = t0, t1
    cc = np.zeros((12, 12))
    cc[:n0 - 4, :n1 - 4] = c
    rec[40:184] = cc.reshape(-1)
    return rec.astype(dtype)


def bias_field_host(rec, hp: int) -> np.ndarray:
    """fp64 [hp,hp]: clip(scale * S, 1 - m, 1 + m) of one record, S evaluated as ctl_aug_bias does (span, fpbspl, 4x4 sum)."""
    rec = np.asarray(rec, dtype=np.float64)
    n0, n1 = int(rec[1]), int(rec[2])
    c = rec[40:184].reshape(12, 12)
    pos = np.arange(hp, dtype=np.float64) - hp // 2
    b0, l0 = _bspline_basis(rec[8:8 + n0], pos)
    b1, l1 = _bspline_basis(rec[24:24 + n1], pos)
    s = np.zeros((hp, hp))
    for i in range(4):
        for j in range(4):
            s += b0[:, i, None] * b1[None, :, j] * c[(l0 + i)[:, None], (l1 + j)[None, :]]
    return np.clip(rec[3] * s, 1.0 - rec[4], 1.0 + rec[4])


def bias_noise_host(seeds, hp: int, wp: int) -> np.ndarray:
    """N of ctl_aug_bias without a noise array: fp64 [n,1,hp,wp] standard normals, Box-Muller on the two uniforms of the counter hash."""
    seeds = np.asarray(seeds, dtype=np.int64).astype(np.uint64).reshape(-1)
    n = seeds.shape[0]
    sample = np.arange(n, dtype=np.uint64).reshape(n, 1) << np.uint64(32)
    pixel = np.arange(hp * wp, dtype=np.uint64).reshape(1, -1)
    h = _mix(seeds.reshape(n, 1) ^ _mix(sample | pixel))
    u1 = ((h >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).reshape(n, 1, hp, wp)


def bias_host(image, bias, seeds=None, noise=None) -> np.ndarray:
    """ctl_aug_bias in fp64: image [n,1,hp,hp], bias [n,192] (any float dtype) -> fp64 [n,1,hp,hp].  Nothing is rounded on the way."""
    image = np.asarray(image)
    out = image.astype(np.float64)
    bias = np.asarray(bias, dtype=np.float64)
    n, _, hp, wp = image.shape
    check_bias_side(hp, wp)
    hashed = None
    for b in range(n):
        if bias[b, 0] == 0 or not abs(out[b, 0].sum()) > 1e-6:
            continue
        v = out[b, 0] * bias_field_host(bias[b], hp)
        v = (v - v.min()) / (v.max() - v.min() + 1e-8)
        if bias[b, 5] > 0:
            if noise is None:                                 # keyed by the sample's index in the batch, as on the device
                hashed = bias_noise_host(seeds, hp, wp) if hashed is None else hashed
            nz = hashed[b, 0] if noise is None else np.asarray(noise, dtype=np.float64)[b, 0]
            v = np.clip(v + bias[b, 5] * nz, 0.0, 1.0)
        out[b, 0] = v
    return out


# coarse-grid displacement (MyElasticTransformCoarseGrid, _utils/elastic_transform.py:105-172) -- the record of ctl_aug_coarse_field
def coarse_record(m, on: bool = True, dtype=np.float32) -> np.ndarray:
    """One sample's record for ctl_aug_coarse_field ([24]) from its two 3x3 planes m [2,3,3] (rows, cols): the coefficients
    spline_filter(order=3, mode='mirror') of either plane in fp64, the clip bounds [min m, max m], on."""
    from scipy import ndimage
    rec = np.zeros(COARSE_FLOATS, dtype=np.float64)
    if on:
        m = np.asarray(m, dtype=np.float64).reshape(2, 3, 3)
        for a in range(2):
            rec[a * 9:a * 9 + 9] = ndimage.spline_filter(m[a], order=3, mode="mirror", output=np.float64).reshape(-1)
            rec[18 + 2 * a], rec[19 + 2 * a] = m[a].min(), m[a].max()
        rec[22] = 1.0
    return rec.astype(dtype)


def _bspline3(t):
    """Cubic B-spline weights [len(t),4] of the taps floor(s) - 1 .. floor(s) + 2 for t = s - floor(s) (aug_bspline3)."""
    u = 1.0 - t
    return np.stack([u * u * u / 6.0, (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0, (4.0 - 6.0 * u * u + 3.0 * u * u * u) / 6.0, t * t * t / 6.0], axis=-1)


def coarse_field_host(coarse, hp: int, wp: int) -> np.ndarray:
    """ctl_aug_coarse_field in fp64: coarse [n,24] (any float dtype) -> [n,2,hp,wp]: 4x4 taps at ((r + 0.5) 3 / hp - 0.5, (c + 0.5) 3 / wp -
    0.5) with indices mirrored about the first and last sample, clipped to the record's bounds; zeros for a sample that is off."""
    coarse = np.asarray(coarse, dtype=np.float64).reshape(-1, COARSE_FLOATS)
    out = np.zeros((coarse.shape[0], 2, hp, wp))
    taps = []
    for side in (hp, wp):
        s = (np.arange(side, dtype=np.float64) + 0.5) * (3.0 / side) - 0.5
        f = np.floor(s)
        idx = np.mod(f.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 4)
        taps.append((_bspline3(s - f), np.where(idx < 3, idx, 4 - idx)))
    (wy, iy), (wx, ix) = taps
    for b in range(coarse.shape[0]):
        if coarse[b, 22] == 0:
            continue
        for a in range(2):
            c = coarse[b, a * 9:a * 9 + 9].reshape(3, 3)
            val = np.zeros((hp, wp))
            for t in range(4):
                for u in range(4):
                    val += wy[:, t, None] * wx[None, :, u] * c[iy[:, t][:, None], ix[:, u][None, :]]
            out[b, a] = np.clip(val, coarse[b, 18 + 2 * a], coarse[b, 19 + 2 * a])
    return out


def source_coords(matrix, hp: int, wp: int, hc: int, wc: int, field=None) -> np.ndarray:
    """fp64 [n,2,hc,wc]: s = M (p + d(p) - c) + c for every pixel of the crop window."""
    m = np.asarray(matrix, dtype=np.float64)
    cy, cx = crop_offsets(hp, wp, hc, wc)
    pr, pc = np.meshgrid(np.arange(hc, dtype=np.float64) + cy, np.arange(wc, dtype=np.float64) + cx, indexing="ij")
    qr, qc = np.broadcast_to(pr, (m.shape[0], hc, wc)).copy(), np.broadcast_to(pc, (m.shape[0], hc, wc)).copy()
    if field is not None:
        f = np.asarray(field, dtype=np.float64)
        qr += f[:, 0, cy:cy + hc, cx:cx + wc]
        qc += f[:, 1, cy:cy + hc, cx:cx + wc]
    cr, cc = (hp - 1) / 2.0, (wp - 1) / 2.0
    qr -= cr
    qc -= cc
    e = lambda i: m[:, i // 3, i % 3].reshape(-1, 1, 1)
    return np.stack([e(0) * qr + e(1) * qc + e(2) + cr, e(3) * qr + e(4) * qc + e(5) + cc], axis=1)


def _inside(s, hp: int, wp: int) -> np.ndarray:
    """Where a cubic value is read: -0.5 <= s_r <= Hp - 0.5 and -0.5 <= s_c <= Wp - 0.5 (elsewhere the result is 0).  s: [2,hc,wc]"""
    return (s[0] >= -0.5) & (s[0] <= hp - 0.5) & (s[1] >= -0.5) & (s[1] <= wp - 0.5)


def warp_host(image, label, matrix, intensity, crop, field=None, interp="linear", n_class=None):
    """ctl_aug_warp (interp="linear") or ctl_aug_warp_cubic (interp="cubic", with n_class) in fp64: (image fp64 [n,1,hc,wc], label int64
    [n,hc,wc]).  Cubic: map_coordinates(order=3, mode='reflect') of the intensity-mapped image and of every indicator label == k inside
    the array, 0 outside; the label is the largest k whose value is >= 0.5 (_utils/elastic_transform.py:84-92)."""
    from scipy import ndimage
    if interp not in ("linear", "cubic"):
        raise ValueError(f"warp_host: interp must be 'linear' or 'cubic', got {interp!r}")
    if interp == "cubic" and (n_class is None or not 1 <= int(n_class) <= 16):
        raise ValueError(f"warp_host: interp='cubic' needs n_class in 1..16, got {n_class!r}")
    image, label = np.asarray(image, dtype=np.float64), np.asarray(label)
    n, _, hp, wp = image.shape
    hc, wc = int(crop[0]), int(crop[1])
    it = np.asarray(intensity, dtype=np.float64)
    s = source_coords(matrix, hp, wp, hc, wc, field)
    io, lo = np.zeros((n, 1, hc, wc)), np.zeros((n, hc, wc), dtype=np.int64)
    for b in range(n):
        v = np.clip(image[b, 0] * it[b, 0] + it[b, 1], image[b, 0].min(), image[b, 0].max())
        if interp == "cubic":
            inside = _inside(s[b], hp, wp)
            io[b, 0] = np.where(inside, ndimage.map_coordinates(v, s[b], order=3, mode="reflect"), 0.0)
            for k in range(int(n_class)):
                val = ndimage.map_coordinates((label[b] == k).astype(np.float64), s[b], order=3, mode="reflect")
                lo[b][inside & (val >= 0.5)] = k
            continue
        io[b, 0] = ndimage.map_coordinates(v, s[b], order=1, mode="grid-constant", cval=0.0)
        r = np.floor(s[b] + 0.5).astype(np.int64)
        inside = (r[0] >= 0) & (r[0] < hp) & (r[1] >= 0) & (r[1] < wp)
        lo[b] = np.where(inside, label[b][np.clip(r[0], 0, hp - 1), np.clip(r[1], 0, wp - 1)], 0)
    return io, lo


def rescale_host(image, new_min=0.0, new_max=1.0, eps=1e-20):
    """ctl_rescale_intensity per plane in fp64 (basic_operations.py:232-245)."""
    image = np.asarray(image, dtype=np.float64)
    mn, mx = image.min(axis=(-2, -1), keepdims=True), image.max(axis=(-2, -1), keepdims=True)
    return (image - mn) / (mx - mn + eps) * (new_max - new_min) + new_min


def apply_host(image, label, params, noise=None, field=None, interp="linear", n_class=None, bias_noise=None):
    """The whole chain on the host in fp64 numpy / scipy, from the definitions of include/ctl_hip.h: image [n,1,Hp,Wp], label [n,Hp,Wp],
    params as BatchAugmenter.draw returns them -> (image float32 [n,1,Hc,Wc] in [0, 1], label int64 [n,Hc,Wc]).  noise: explicit u
    [n,2,Hp,Wp] in place of the counter hash; field: an explicit displacement in place of the filtered noise or of the coarse-grid field.
    The elastic stage runs only when params carries alpha (a policy with elastic deformation), the coarse-grid stage when it carries
    coarse, the bias pre-pass (bias_host; bias_noise: explicit normals [n,1,Hp,Wp] in place of the hashed ones) when it carries bias: the
    warp and its intensity clamp then read the biased plane.  interp, n_class: as warp_host."""
    image, label = _np(image), _np(label)
    n, _, hp, wp = image.shape
    hc, wc = (int(v) for v in _np(params["crop"]))
    if params.get("bias") is not None:
        image = bias_host(image, _np(params["bias"]), seeds=None if params.get("bias_seed") is None else _np(params["bias_seed"]),
                          noise=None if bias_noise is None else _np(bias_noise))
    if field is None and params.get("alpha") is not None:
        field = elastic_field_host(_np(params["alpha"]), _np(params["sigma"]), hp, wp, seeds=_np(params["seed"]), noise=None if noise is None else _np(noise))
    elif field is None and params.get("coarse") is not None:
        field = coarse_field_host(_np(params["coarse"]), hp, wp)
    elif field is not None:
        field = _np(field)
    io, lo = warp_host(image, label, _np(params["matrix"]), _np(params["intensity"]), (hc, wc), field, interp=interp, n_class=n_class)
    return rescale_host(io).astype(np.float32), lo


# ---------------------------------------------------------------------------------------------- the augmenter
DEVICE_KEYS = ("matrix", "intensity", "alpha", "sigma", "seed")
# with the entries of the stages that only a config dict switches on (absent for every policy name)
CONFIG_DEVICE_KEYS = DEVICE_KEYS + ("bias", "bias_seed", "coarse")


def _shares_memory(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Do the address ranges of two contiguous device tensors overlap?"""
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


class BatchAugmenter:
    """`Transformations(policy).get_transformation()['train']` (transform.py:13-86) for a batch on the device.

    draw(n, hp, wp)   per-sample parameters from a seeded numpy Generator, as small CPU tensors:
                        flip [n,2] bool (horizontal, vertical), theta [n] deg, translate [n,2] fractions (height, width), zoom [n,2]
                        (rows, cols), choice [n] deg, intensity_on / elastic_on [n] bool, contrast, brightness [n]   -- what was drawn
                        matrix [n,2,3] f32, intensity [n,2] f32, alpha / sigma [n] f32, seed [n] i64, crop [2] i64   -- what apply reads
                      alpha / sigma / seed are None for a policy without elastic deformation; alpha is 0 where elastic is off.
    apply(image, label, params, out=None)
                      device tensors: device-only, no host synchronisation, capturable in a graph (params' DEVICE_KEYS entries must
                      then be device tensors whose content is refreshed between replays; CONFIG_DEVICE_KEYS with from_config).  6 launches with an elastic policy (field 2,
                      warp 2, rescale 2), else 4.  out = (image_out, label_out) must not share memory with image or label.
                      numpy arrays: apply_host.
    __call__(image, label)   draw, a pinned non-blocking upload of the parameters, apply.

    interp="cubic" (with num_classes, 1..16) reads image and label through a cubic spline as upstream's elastic stage does: the image by
    map_coordinates(order=3, mode='reflect'), the label as per-class indicator maps thresholded at 0.5, zero outside the array; still one
    resampling.  draw does not depend on interp.  The warp then takes 4 launches (min / max partials, prefilter rows, prefilter columns,
    gather): 8 launches per batch with an elastic policy, else 6, whatever n is.

    from_config(config, crop_size, ...) builds the chain from upstream's config dict and adds two stages no policy name has:
      bias field   (perturb_v2_prob > 0) a pre-pass that writes a new [n,1,Hp,Wp] image (ctl_aug_bias, +2 launches); the warp's contrast /
                   brightness clamp then uses the min / max of the biased plane, as upstream applies brightness after the perturbation.
                   Hp == Wp, even, 128..512.
      coarse grid  (elastic_probv2 > 0) the displacement of the 3x3 coarse grid in place of the Gaussian one (ctl_aug_coarse_field, 1 launch
                   where the Gaussian field takes 2).
    draw then also returns bias_on / coarse_on [n] bool, bias_knots [n,k,k] f32 and coarse_normals [n,2,3,3] f64 (what was drawn) and
    bias [n,192] f32, bias_seed [n] i64, coarse [n,24] f32 (what apply reads: CONFIG_DEVICE_KEYS); a stage that is not there adds no entry.
    These draws come after all the others, so a config without either stage consumes the generator exactly as its policy name does."""

    def __init__(self, policy: str, crop_size, seed: int = 0, interp: str = "linear", num_classes=None):
        self._setup(policy, get_policy(policy), crop_size, seed, interp, num_classes)

    @classmethod
    def from_config(cls, config: dict, crop_size, seed: int = 0, interp: str = "linear", num_classes=None):
        """The chain of `Transformations.get_transform(config)` (transform.py:46-86) for upstream's config dict: the keys of no_aug()
        (transform.py:114-144), missing ones taking its values; an unknown key raises KeyError.  gamma_prob, gamma_range and
        ms_control_point_spacing are accepted and ignored, as upstream ignores them: get_transform has no gamma stage, and the V2
        constructor overwrites the spacing with [64] (intensity_transform.py:404).  perturb_prob > 0 (MyRandomPurtarbation, V1) raises
        NotImplementedError; elastic_prob > 0 together with elastic_probv2 > 0 raises ValueError."""
        self = cls.__new__(cls)
        self._setup(None, policy_from_config(config), crop_size, seed, interp, num_classes)
        return self

    def _setup(self, name, policy, crop_size, seed, interp, num_classes):
        if interp not in ("linear", "cubic"):
            raise ValueError(f"BatchAugmenter: interp must be 'linear' or 'cubic', got {interp!r}")
        if interp == "cubic" and (num_classes is None or not 1 <= int(num_classes) <= 16):
            raise ValueError(f"BatchAugmenter: interp='cubic' needs num_classes in 1..16 (one indicator plane per class), got {num_classes!r}")
        self.interp = interp
        self.num_classes = None if num_classes is None else int(num_classes)
        self.policy_name = name
        self.policy = policy
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.rng = np.random.default_rng(seed)
        self.elastic = self.policy["elastic_prob"] > 0.0
        self.coarse = self.policy.get("coarse_prob", 0.0) > 0.0
        self.bias = self.policy.get("bias_prob", 0.0) > 0.0

    def draw(self, n: int, hp: int, wp: int) -> dict:
        p, g = self.policy, self.rng
        n, hp, wp = int(n), int(hp), int(wp)
        if self.crop_size[0] > hp or self.crop_size[1] > wp:
            raise ValueError(f"BatchAugmenter: crop {self.crop_size} is larger than the input {(hp, wp)}")
        if self.bias:
            check_bias_side(hp, wp)
        fh, fv, fp = p["flip"]
        flip = np.stack([(g.random(n) < fp) & bool(fh), (g.random(n) < fp) & bool(fv)], axis=1)
        theta = g.uniform(-p["rotate"], p["rotate"], n) if p["rotate"] else np.zeros(n)
        translate = np.stack([g.uniform(-p["shift"][0], p["shift"][0], n) if p["shift"][0] else np.zeros(n),
                              g.uniform(-p["shift"][1], p["shift"][1], n) if p["shift"][1] else np.zeros(n)], axis=1)
        lo, hi = p["scale"]
        zoom = g.uniform(lo, hi, (n, 2)) if hi > lo else np.full((n, 2), float(lo))
        choice = g.choice(np.asarray(p["rotate_groups"], dtype=np.float64), n) if p["rotate_groups"] else np.zeros(n)
        intensity_on = g.random(n) < p["intensity_prob"]
        contrast = np.where(intensity_on, g.uniform(*CONTRAST_RANGE, n), 1.0)
        brightness = np.where(intensity_on, g.uniform(*BRIGHTNESS_RANGE, n), 0.0)
        elastic_on = g.random(n) < p["elastic_prob"]
        matrix = compose_matrix(flip, theta, translate, zoom, choice, hp, wp, shear=np.full(n, p["shear"]))
        out = {"flip": torch.from_numpy(flip), "theta": torch.from_numpy(theta), "translate": torch.from_numpy(translate),
               "zoom": torch.from_numpy(zoom), "choice": torch.from_numpy(choice), "intensity_on": torch.from_numpy(intensity_on),
               "contrast": torch.from_numpy(contrast), "brightness": torch.from_numpy(brightness), "elastic_on": torch.from_numpy(elastic_on),
               "matrix": torch.from_numpy(matrix.astype(np.float32)),
               "intensity": torch.from_numpy(np.stack([contrast, brightness], axis=1).astype(np.float32)),
               "alpha": None, "sigma": None, "seed": None, "crop": torch.tensor(self.crop_size, dtype=torch.int64)}
        if self.elastic:
            alpha = np.where(elastic_on, hp * g.uniform(*ALPHA_RANGE, n), 0.0)
            sigma = hp * g.uniform(*SIGMA_RANGE, n) * SIGMA_FACTOR
            out["alpha"] = torch.from_numpy(alpha.astype(np.float32))
            out["sigma"] = torch.from_numpy(sigma.astype(np.float32))
            out["seed"] = torch.from_numpy(g.integers(0, 2 ** 63 - 1, n, dtype=np.int64))
        if self.bias:
            m, k = p["bias_m"], bias_grid(hp)[2].shape[0]
            bias_on = g.random(n) < p["bias_prob"]
            knots = 1 + np.float32(g.uniform(-m, m, (n, k, k)))           # 1 + float32(U(-m, m)), intensity_transform.py:463-464
            out["bias_on"], out["bias_knots"] = torch.from_numpy(bias_on), torch.from_numpy(knots)
            out["bias"] = torch.from_numpy(np.stack([bias_record(knots[b], hp, m, p["bias_eps"], on=bool(bias_on[b])) for b in range(n)]))
            out["bias_seed"] = torch.from_numpy(g.integers(0, 2 ** 63 - 1, n, dtype=np.int64))
        if self.coarse:
            coarse_on = g.random(n) < p["coarse_prob"]
            normals = g.normal(0.0, COARSE_SIGMA, (n, 2, 3, 3))
            out["coarse_on"], out["coarse_normals"] = torch.from_numpy(coarse_on), torch.from_numpy(normals)
            out["coarse"] = torch.from_numpy(np.stack([coarse_record(normals[b], on=bool(coarse_on[b])) for b in range(n)]))
        return out

    @staticmethod
    def upload(params: dict, device) -> dict:
        """params with the entries apply reads copied to `device` through pinned memory, without blocking the host."""
        out = dict(params)
        for k in CONFIG_DEVICE_KEYS:
            if params.get(k) is not None and not params[k].is_cuda:
                out[k] = params[k].pin_memory().to(device, non_blocking=True)
        return out

    def apply(self, image, label, params: dict, out=None):
        if isinstance(image, np.ndarray):
            return apply_host(image, label, params, interp=self.interp, n_class=self.num_classes)
        ops.require_gpu(image, label, *(params.get(k) for k in CONFIG_DEVICE_KEYS))
        n, _, hp, wp = image.shape
        crop = self.crop_size
        if out is not None and _shares_memory(out[0], image):
            raise ValueError("BatchAugmenter.apply: out[0] shares memory with image")
        if params.get("bias") is not None:
            image = ops.aug_bias_field(image, params["bias"], seed=params["bias_seed"])
        field = None
        if params.get("alpha") is not None:
            field = ops.aug_elastic_field(n, hp, wp, params["alpha"], params["sigma"], params["seed"], device=image.device)
        elif params.get("coarse") is not None:
            field = ops.aug_coarse_field(n, hp, wp, params["coarse"], device=image.device)
        warped, lab = ops.aug_warp(image, label, params["matrix"], params["intensity"], crop, field=field,
                                   out=None if out is None else (torch.empty_like(out[0]), out[1]), interp=self.interp,
                                   n_class=self.num_classes if self.interp == "cubic" else None)
        return ops.rescale_intensity(warped, 0.0, 1.0, out=None if out is None else out[0]), lab

    def __call__(self, image, label):
        n, _, hp, wp = image.shape
        params = self.draw(n, hp, wp)
        if isinstance(image, torch.Tensor):
            params = self.upload(params, image.device)
        return self.apply(image, label, params)
