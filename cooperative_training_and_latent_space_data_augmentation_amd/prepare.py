"""Patient volume preparation on the device: raw array + spacing in, network-ready tensors out.

Mirror of what upstream does per volume on the host before a tensor reaches the network:
`load_img_label_from_path` (medseg/common_utils/basic_operations.py:337-365) without the disk -- resample the in-plane spacing
(`resample_by_spacing`, medseg/dataset_loader/dataset_utils.py:39-63), then `normalize_minmax_data` (dataset_utils.py:15-36) -- and
`get_patient_data_for_testing` (medseg/dataset_loader/cardiac_ACDC_dataset.py:204-232) on top of it: centre crop / pad and the
per-slice min-max rescale.  A numpy input is uploaded once; everything after that is device work without a readback.

The `*_host` functions are the same statements as plain numpy (fp64 where the device computes in fp64, float32 with one rounding per
operation where it computes in float32).  They are what the device results are tested against; scipy appears only in the tests that
cross-check them.

The way back is recorded too: `geometry` keeps what the forward trip did to the in-plane grid (resampling ratios, sizes, crop offset),
and `restore_prediction` puts a window-grid prediction back on the patient's native grid with it (ops.restore_scores /
ops.restore_labels; `restore_scores_host` / `restore_labels_host` are the numpy statements)."""
import collections

import numpy as np
import torch

from . import ops

F32 = np.float32


# ------------------------------------------------------------------------------------------------ device path
def _upload(a, dtype=None):
    """numpy array or tensor -> device tensor (one copy), cast to dtype if given."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    dev = torch.device("cuda", torch.cuda.current_device())
    return t.to(device=dev, dtype=dtype) if dtype is not None else t.to(device=dev)


def load_volume(image, label=None, spacing=None, new_spacing=None, normalize=False):
    """`load_img_label_from_path` (basic_operations.py:337-365) from arrays instead of files: image [n,h,w] (cast to float32, as
    sitk.Cast does), label [n,h,w] of an integer type or None, spacing / new_spacing (x, y, z) as SimpleITK orders them.  With
    new_spacing the in-plane axes are resampled first (ops.resample_inplane; new_spacing[2] must be negative), then, with normalize,
    the whole volume is clipped to its 2 / 98 percentiles and scaled (ops.percentile_normalize, form "minmax").
    -> (image float32 [n,h',w'], label or None, spacing_out) on the device; a uint8 label stays uint8, any other becomes int64."""
    image_d = _upload(image, torch.float32)
    label_d = None
    if label is not None:
        keep = (label.dtype == np.uint8) if isinstance(label, np.ndarray) else (label.dtype == torch.uint8)
        label_d = _upload(label, torch.uint8 if keep else torch.int64)
    if image_d.dim() != 3 or (label_d is not None and label_d.shape != image_d.shape):
        raise ValueError("load_volume: expected an [n,h,w] image and a label of the same shape")
    spacing_out = None if spacing is None else tuple(float(v) for v in spacing)
    if new_spacing is not None:
        if spacing is None:
            raise ValueError("load_volume: new_spacing needs the spacing of the input")
        image_d, label_d, spacing_out = ops.resample_inplane(image_d, spacing, new_spacing, label=label_d)
    if normalize:
        image_d = ops.percentile_normalize(image_d.contiguous(), (2.0, 98.0), form="minmax", segments=1)
    return image_d, label_d, spacing_out


class Geometry(collections.namedtuple("Geometry", "native_hw resampled_hw window_hw offset q spacing")):
    """What the forward trip (ops.resample_inplane, then ops.crop_or_pad) did to the in-plane grid of one patient, immutable:
    native_hw (h, w); resampled_hw (h', w'); window_hw (Hc, Wc); offset (dy, dx) = floor((resampled - window) / 2), negative when the
    window was padded; q (q_h, q_w) = native spacing / new spacing, exactly (1.0, 1.0) when nothing was resampled; spacing = the native
    (x, y, z) or None.  Native index i sits at resampled-grid coordinate i * q and at window coordinate i * q - offset."""
    __slots__ = ()


def geometry(n, h, w, spacing=None, new_spacing=None, crop_size=None):
    """The Geometry of a [n,h,w] volume prepared with (spacing, new_spacing, crop_size), from ops.resample_geometry: sizes by upstream's
    rounding, q = spacing / new_spacing per axis (one fp64 division each; entry 0 of a spacing is the WIDTH axis), identity when no
    new_spacing is given or upstream's sum rule says so.  crop_size None: the window is the resampled size."""
    h, w = int(h), int(w)
    rh, rw, q = h, w, (1.0, 1.0)
    if new_spacing is not None:
        if spacing is None:
            raise ValueError("geometry: new_spacing needs the spacing of the input")
        new_h, new_w, _, _, identity = ops.resample_geometry(n, h, w, spacing, new_spacing)
        if not identity:
            rh, rw = new_h, new_w
            q = (float(spacing[1]) / float(new_spacing[1]), float(spacing[0]) / float(new_spacing[0]))
    hc, wc = (rh, rw) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    return Geometry((h, w), (rh, rw), (hc, wc), ((rh - hc) // 2, (rw - wc) // 2), q,
                    None if spacing is None else tuple(float(v) for v in spacing))


def prepare_patient(image, label, spacing=None, new_spacing=None, normalize=False, crop_size=None, normalize_2D=True, want_geometry=False):
    """`get_patient_data_for_testing` (cardiac_ACDC_dataset.py:204-232) on the device: load_volume, then ops.crop_or_pad to crop_size
    ([H', W'], None: the size stays), then ops.rescale_intensity per slice (normalize_2D).
    -> {'image': float32 [n,1,H',W'], 'label': int64 [n,H',W']} on the device, what TestSegmentationNetwork.evaluate takes.
    want_geometry adds 'geometry' (the Geometry of the trip) and 'native_label' (the label as uploaded, before resampling): what
    TestSegmentationNetwork(native_grid=True) and restore_prediction need."""
    if want_geometry:
        keep = (label.dtype == np.uint8) if isinstance(label, np.ndarray) else (label.dtype == torch.uint8)
        native = _upload(label, torch.uint8 if keep else torch.int64)                  # load_volume's upload, done once here
        geo = geometry(*native.shape, spacing=spacing, new_spacing=new_spacing, crop_size=crop_size)
        pack = prepare_patient(image, native, spacing=spacing, new_spacing=new_spacing, normalize=normalize, crop_size=crop_size,
                               normalize_2D=normalize_2D)
        pack.update(geometry=geo, native_label=native)
        return pack
    image_d, label_d, _ = load_volume(image, label, spacing=spacing, new_spacing=new_spacing, normalize=normalize)
    if crop_size is not None:
        image_d, label_d = ops.crop_or_pad(image_d, crop_size, label=label_d)
    image_d = image_d.contiguous().unsqueeze(1)
    if normalize_2D:
        image_d = ops.rescale_intensity(image_d, 0.0, 1.0)
    return {"image": image_d, "label": label_d.long()}


def restore_prediction(scores_or_labels, geometry, mode="logit", want_soft=False):
    """A window-grid prediction back on the native grid of `geometry`, on the device: float32 [n,C,Hc,Wc] scores go through
    ops.restore_scores (-> uint8 label [n,h,w], or (label, soft) with want_soft), uint8 [n,Hc,Wc] labels through ops.restore_labels."""
    t = scores_or_labels
    if t.dtype == torch.float32 and t.dim() == 4:
        return ops.restore_scores(t, geometry, mode=mode, want_soft=want_soft)
    if t.dtype == torch.uint8 and t.dim() == 3:
        if want_soft:
            raise ValueError("restore_prediction: a label volume has no soft prediction")
        return ops.restore_labels(t, geometry)
    raise ValueError(f"restore_prediction: expected float32 [n,C,Hc,Wc] scores or uint8 [n,Hc,Wc] labels, got {t.dtype} {tuple(t.shape)}")


# ------------------------------------------------------------------------------------------------ host statements
def _segments(x, segments):
    x = np.ascontiguousarray(x, dtype=F32)
    if segments < 1 or x.size == 0 or x.size % segments:
        raise ValueError(f"{x.size} elements do not split into {segments} equal, non-empty segments")
    return x.reshape(segments, -1)


def _lerp_host(a, b, g):
    """numpy's _lerp on float32 neighbours in fp64, rounded once to float32"""
    a, b = np.float64(a), np.float64(b)
    d = b - a
    return F32(a + d * g if g < 0.5 else b - d * (1.0 - g))


def percentile_host(x, q, segments=1):
    """np.percentile(x.astype(float64), q) per segment, rounded once to float32, from the definition: sort, the two order statistics
    around the virtual index (n - 1) * (q / 100), numpy's _lerp in fp64.  x: float32 without NaN.  -> float32 [segments, len(q)],
    or a float32 scalar for one segment and a scalar q."""
    scalar = np.ndim(q) == 0 and segments == 1
    qs = np.asarray(q, dtype=np.float64).reshape(-1)
    s = np.sort(_segments(x, segments), axis=1)
    out = np.empty((segments, qs.size), dtype=F32)
    for j, qq in enumerate(qs):
        k, ku, g = ops.percentile_index(s.shape[1], qq)
        for i in range(segments):
            out[i, j] = _lerp_host(s[i, k], s[i, ku], g)
    return out[0, 0] if scalar else out


def percentile_normalize_host(x, q=(2.0, 98.0), form="minmax", segments=1, new_min=0.0, new_max=1.0, want_bounds=False):
    """ops.percentile_normalize in numpy float32, one rounding per operation (the formulas are in its docstring)."""
    if form not in ops.PERCENTILE_FORMS:
        raise ValueError(f"form {form!r}")
    shape = np.shape(x)
    v = _segments(x, segments).copy()
    bounds = percentile_host(v, list(q), segments).reshape(segments, 2)
    lo, hi = bounds[:, :1], bounds[:, 1:]
    with np.errstate(all="ignore"):
        if form == "minmax":
            v = np.where(v < lo, lo, v)
            v = np.where(v > hi, hi, v)
            out = (v - lo) / ((F32(1e-10) + hi) - lo)
        else:
            v = np.where(v <= lo, lo, v)
            v = np.where(v >= hi, hi, v)
            a = (F32(new_max) - F32(new_min)) / ((hi - lo) + F32(1e-8))
            b = F32(new_max) - a * hi
            out = v * a + b
    out = out.astype(F32, copy=False).reshape(shape)
    assert out.dtype == F32
    return (out, bounds) if want_bounds else out


def resample_inplane_host(image, spacing, new_spacing, label=None):
    """ops.resample_inplane in numpy: fp64 coordinates j * r, linear over the two neighbours per axis (rows first) rounded once to
    float32, nearest = floor(c + 0.5) for the label, 0 where c >= size - 0.5 on either axis.  -> (image, label, spacing_out)."""
    n, h, w = image.shape
    new_h, new_w, r_h, r_w, identity = ops.resample_geometry(n, h, w, spacing, new_spacing)
    if identity:
        return image, label, tuple(float(v) for v in spacing)
    cy, cx = np.arange(new_h, dtype=np.float64) * r_h, np.arange(new_w, dtype=np.float64) * r_w
    inside = (cy < h - 0.5)[:, None] & (cx < w - 0.5)[None, :]
    fy, fx = np.floor(cy), np.floor(cx)
    ty, tx = (cy - fy)[None, :, None], (cx - fx)[None, None, :]
    y0, x0 = np.clip(fy.astype(np.int64), 0, h - 1), np.clip(fx.astype(np.int64), 0, w - 1)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    src = np.asarray(image, dtype=F32).astype(np.float64)
    top = src[:, y0][:, :, x0] * (1.0 - tx) + src[:, y0][:, :, x1] * tx
    bot = src[:, y1][:, :, x0] * (1.0 - tx) + src[:, y1][:, :, x1] * tx
    out = np.where(inside[None], top * (1.0 - ty) + bot * ty, 0.0).astype(F32)
    label_out = None
    if label is not None:
        label = np.asarray(label)
        yn = np.clip(np.floor(cy + 0.5).astype(np.int64), 0, h - 1)
        xn = np.clip(np.floor(cx + 0.5).astype(np.int64), 0, w - 1)
        label_out = np.where(inside[None], label[:, yn][:, :, xn], 0).astype(label.dtype)
    return out, label_out, (float(new_spacing[0]), float(new_spacing[1]), float(spacing[2]))


def _crop_or_pad_host(a, crop_size):
    """centre crop / zero pad of [n,h,w] (basic_operations.py:173-220): source index = dst + floor((size - new) / 2), 0 outside"""
    n, h, w = a.shape
    nh, nw = int(crop_size[0]), int(crop_size[1])
    ys, xs = np.arange(nh) + (h - nh) // 2, np.arange(nw) + (w - nw) // 2
    ok = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    got = a[:, np.clip(ys, 0, h - 1)][:, :, np.clip(xs, 0, w - 1)]
    return np.where(ok[None], got, 0).astype(a.dtype)


def prepare_patient_host(image, label, spacing=None, new_spacing=None, normalize=False, crop_size=None, normalize_2D=True):
    """prepare_patient in numpy: {'image': float32 [n,1,H',W'], 'label': int64 [n,H',W']}."""
    image, label = np.asarray(image, dtype=F32), np.asarray(label)
    if new_spacing is not None:
        image, label, _ = resample_inplane_host(image, spacing, new_spacing, label=label)
    if normalize:
        image = percentile_normalize_host(image, (2.0, 98.0), form="minmax", segments=1)
    if crop_size is not None:
        image, label = _crop_or_pad_host(image, crop_size), _crop_or_pad_host(label, crop_size)
    if normalize_2D:                                           # ctl_rescale_intensity: ((x - mn) / ((mx - mn) + eps)) * range + new_min in float32
        mn, mx = image.min(axis=(1, 2), keepdims=True), image.max(axis=(1, 2), keepdims=True)
        with np.errstate(all="ignore"):
            image = ((image - mn) / ((mx - mn) + F32(1e-20))) * F32(1.0) + F32(0.0)
    return {"image": np.ascontiguousarray(image[:, None], dtype=F32), "label": label.astype(np.int64)}


def restore_coordinates_host(geometry):
    """Per axis of the native grid: the window coordinates u = i * q - offset (fp64) and which native voxels are inside
    (i * q < resampled - 0.5 and -0.5 <= u < window - 0.5 on both axes).  -> (u_y [h], u_x [w], inside [h,w])."""
    out = []
    for a in (0, 1):
        c = np.arange(geometry.native_hw[a], dtype=np.float64) * np.float64(geometry.q[a])
        u = c - np.float64(geometry.offset[a])
        out.append((u, (c < geometry.resampled_hw[a] - 0.5) & (u >= -0.5) & (u < geometry.window_hw[a] - 0.5)))
    return out[0][0], out[1][0], out[0][1][:, None] & out[1][1][None, :]


def restore_values_host(scores, geometry, mode="logit"):
    """The fp64 values ctl_restore_scores takes its arg-max over: scores float32 [n,C,Hc,Wc] -> (v float64 [n,C,h,w], inside [h,w]).
    Tap value = the score (mode "logit") or the pixel's softmax exp(x - max) / sum (mode "prob", summed in ascending class order);
    f = floor(u), t = u - f, taps clamp(f) and clamp(f + 1) separately; top = s00 (1 - tx) + s01 tx, bot likewise, v = top (1 - ty) +
    bot ty.  Outside voxels hold 0 (logit) or (1, 0, ..., 0) (prob)."""
    if mode not in ops.RESTORE_MODES:
        raise ValueError(f"mode {mode!r}")
    s = np.asarray(scores, dtype=F32).astype(np.float64)
    n, c, hc, wc = s.shape
    if (hc, wc) != tuple(geometry.window_hw):
        raise ValueError(f"the scores' window {(hc, wc)} is not the geometry's {tuple(geometry.window_hw)}")
    if mode == "prob":
        e = np.exp(s - s.max(axis=1, keepdims=True))
        z = e[:, 0]
        for k in range(1, c):
            z = z + e[:, k]
        s = e / z[:, None]
    uy, ux, inside = restore_coordinates_host(geometry)
    fy, fx = np.floor(uy), np.floor(ux)
    ty, tx = (uy - fy)[None, None, :, None], (ux - fx)[None, None, None, :]
    y0, x0 = np.clip(fy.astype(np.int64), 0, hc - 1), np.clip(fx.astype(np.int64), 0, wc - 1)
    y1, x1 = np.clip(fy.astype(np.int64) + 1, 0, hc - 1), np.clip(fx.astype(np.int64) + 1, 0, wc - 1)
    top = s[:, :, y0][:, :, :, x0] * (1.0 - tx) + s[:, :, y0][:, :, :, x1] * tx
    bot = s[:, :, y1][:, :, :, x0] * (1.0 - tx) + s[:, :, y1][:, :, :, x1] * tx
    v = top * (1.0 - ty) + bot * ty
    outside = np.zeros(c, dtype=np.float64)
    if mode == "prob":
        outside[0] = 1.0
    return np.where(inside[None, None], v, outside[None, :, None, None]), inside


def restore_scores_host(scores, geometry, mode="logit", want_soft=False):
    """ops.restore_scores in numpy: label uint8 [n,h,w] = the lowest class with the largest fp64 value (0 outside), and with want_soft
    the values rounded once to float32 [n,C,h,w]."""
    v, inside = restore_values_host(scores, geometry, mode)
    label = np.where(inside[None], np.argmax(v, axis=1), 0).astype(np.uint8)
    return (label, v.astype(F32)) if want_soft else label


def restore_labels_host(labels, geometry):
    """ops.restore_labels in numpy: the window pixel at clamp(floor(u + 0.5), 0, size - 1) per axis, 0 outside."""
    labels = np.asarray(labels)
    n, hc, wc = labels.shape
    if (hc, wc) != tuple(geometry.window_hw):
        raise ValueError(f"the labels' window {(hc, wc)} is not the geometry's {tuple(geometry.window_hw)}")
    uy, ux, inside = restore_coordinates_host(geometry)
    yn = np.clip(np.floor(uy + 0.5).astype(np.int64), 0, hc - 1)
    xn = np.clip(np.floor(ux + 0.5).astype(np.int64), 0, wc - 1)
    return np.where(inside[None], labels[:, yn][:, :, xn], 0).astype(labels.dtype)
