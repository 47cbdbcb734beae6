"""Training augmentation of a batch on the device (medseg/dataset_loader/transform.py:46-86, which upstream runs per slice on the host
inside DataLoader workers): flip, contrast / brightness, random affine, choice rotation, elastic deformation, centre crop, min-max
normalisation.  The parameters of every sample are drawn on the host (a few floats); the pixels never leave the device, and image and
label are resampled once.  The semantics are written out in include/ctl_hip.h next to ctl_aug_field / ctl_aug_warp; `apply_host` states
them again in fp64 numpy / scipy and is the host path for numpy inputs.

    aug = BatchAugmenter("ACDC_affine_elastic_intensity", crop_size=(192, 192), seed=0)
    image, label = aug(image, label)          # [n,1,Hp,Wp] float32, [n,Hp,Wp] int64 on the device -> [n,1,192,192], [n,192,192]

BatchAugmenter(..., interp="cubic", num_classes=K) reads image and label through upstream's cubic spline (ctl_aug_warp_cubic) in place of
bilinear / nearest; the default is unchanged.
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
    """splitmix64 finaliser on uint64 arrays (aug_mix of csrc/ctl_aug.hip)."""
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


def apply_host(image, label, params, noise=None, field=None, interp="linear", n_class=None):
    """The whole chain on the host in fp64 numpy / scipy, from the definitions of include/ctl_hip.h: image [n,1,Hp,Wp], label [n,Hp,Wp],
    params as BatchAugmenter.draw returns them -> (image float32 [n,1,Hc,Wc] in [0, 1], label int64 [n,Hc,Wc]).  noise: explicit u
    [n,2,Hp,Wp] in place of the counter hash; field: an explicit displacement in place of the filtered noise.  The elastic stage runs
    only when params carries alpha (a policy with elastic deformation).  interp, n_class: as warp_host."""
    image, label = _np(image), _np(label)
    n, _, hp, wp = image.shape
    hc, wc = (int(v) for v in _np(params["crop"]))
    if field is None and params.get("alpha") is not None:
        field = elastic_field_host(_np(params["alpha"]), _np(params["sigma"]), hp, wp, seeds=_np(params["seed"]), noise=None if noise is None else _np(noise))
    elif field is not None:
        field = _np(field)
    io, lo = warp_host(image, label, _np(params["matrix"]), _np(params["intensity"]), (hc, wc), field, interp=interp, n_class=n_class)
    return rescale_host(io).astype(np.float32), lo


# ---------------------------------------------------------------------------------------------- the augmenter
DEVICE_KEYS = ("matrix", "intensity", "alpha", "sigma", "seed")


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
                      then be device tensors whose content is refreshed between replays).  6 launches with an elastic policy (field 2,
                      warp 2, rescale 2), else 4.  out = (image_out, label_out) must not share memory with image or label.
                      numpy arrays: apply_host.
    __call__(image, label)   draw, a pinned non-blocking upload of the parameters, apply.

    interp="cubic" (with num_classes, 1..16) reads image and label through a cubic spline as upstream's elastic stage does: the image by
    map_coordinates(order=3, mode='reflect'), the label as per-class indicator maps thresholded at 0.5, zero outside the array; still one
    resampling.  draw does not depend on interp.  The warp then takes 4 launches (min / max partials, prefilter rows, prefilter columns,
    gather): 8 launches per batch with an elastic policy, else 6, whatever n is."""

    def __init__(self, policy: str, crop_size, seed: int = 0, interp: str = "linear", num_classes=None):
        if interp not in ("linear", "cubic"):
            raise ValueError(f"BatchAugmenter: interp must be 'linear' or 'cubic', got {interp!r}")
        if interp == "cubic" and (num_classes is None or not 1 <= int(num_classes) <= 16):
            raise ValueError(f"BatchAugmenter: interp='cubic' needs num_classes in 1..16 (one indicator plane per class), got {num_classes!r}")
        self.interp = interp
        self.num_classes = None if num_classes is None else int(num_classes)
        self.policy_name = policy
        self.policy = get_policy(policy)
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.rng = np.random.default_rng(seed)
        self.elastic = self.policy["elastic_prob"] > 0.0

    def draw(self, n: int, hp: int, wp: int) -> dict:
        p, g = self.policy, self.rng
        n, hp, wp = int(n), int(hp), int(wp)
        if self.crop_size[0] > hp or self.crop_size[1] > wp:
            raise ValueError(f"BatchAugmenter: crop {self.crop_size} is larger than the input {(hp, wp)}")
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
        return out

    @staticmethod
    def upload(params: dict, device) -> dict:
        """params with the entries apply reads copied to `device` through pinned memory, without blocking the host."""
        out = dict(params)
        for k in DEVICE_KEYS:
            if params.get(k) is not None and not params[k].is_cuda:
                out[k] = params[k].pin_memory().to(device, non_blocking=True)
        return out

    def apply(self, image, label, params: dict, out=None):
        if isinstance(image, np.ndarray):
            return apply_host(image, label, params, interp=self.interp, n_class=self.num_classes)
        ops.require_gpu(image, label, *(params.get(k) for k in DEVICE_KEYS))
        n, _, hp, wp = image.shape
        crop = self.crop_size
        if out is not None and _shares_memory(out[0], image):
            raise ValueError("BatchAugmenter.apply: out[0] shares memory with image")
        field = None
        if params.get("alpha") is not None:
            field = ops.aug_elastic_field(n, hp, wp, params["alpha"], params["sigma"], params["seed"], device=image.device)
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
