"""Validation metrics used by `evaluate` (medseg/common_utils/metrics.py:12-54) and Dice (measure.py:52-99)."""
import numpy as np


class runningScore(object):
    """Confusion-matrix accumulator: overall / mean accuracy, mean IoU, frequency-weighted accuracy."""

    def __init__(self, n_classes):
        self.n_classes = n_classes
        self.confusion_matrix = np.zeros((n_classes, n_classes))

    def _fast_hist(self, label_true, label_pred, n_class):
        keep = (label_true >= 0) & (label_true < n_class)
        idx = n_class * label_true[keep].astype(int) + label_pred[keep].astype(int)
        return np.bincount(idx, minlength=n_class ** 2).reshape(n_class, n_class)

    def update(self, label_trues, label_preds):
        """Device tensors (both on the GPU) are accumulated by the HIP kernel into an int64 matrix that stays on the device: no
        host round trip per batch; numpy inputs follow the upstream host path."""
        import torch
        if torch.is_tensor(label_trues) and torch.is_tensor(label_preds) and label_trues.is_cuda and label_preds.is_cuda:
            from . import ops
            self._dev_hist = ops.confusion_hist(label_trues, label_preds, self.n_classes, getattr(self, "_dev_hist", None))
            return
        for lt, lp in zip(label_trues, label_preds):
            self.confusion_matrix += self._fast_hist(np.asarray(lt).flatten(), np.asarray(lp).flatten(), self.n_classes)

    def _total(self):
        h = self.confusion_matrix
        if getattr(self, "_dev_hist", None) is not None:
            h = h + self._dev_hist.cpu().numpy().astype(np.float64)          # the one synchronisation of an evaluation
        return h

    def get_scores(self):
        h = self._total()
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.diag(h).sum() / h.sum()
            acc_cls = np.nanmean(np.diag(h) / h.sum(axis=1))
            iu = np.diag(h) / (h.sum(axis=1) + h.sum(axis=0) - np.diag(h))
            freq = h.sum(axis=1) / h.sum()
        return ({"Overall Acc: \t": acc, "Mean Acc : \t": acc_cls, "FreqW Acc : \t": (freq[freq > 0] * iu[freq > 0]).sum(),
                 "Mean IoU : \t": np.nanmean(iu)}, dict(zip(range(self.n_classes), iu)))

    def reset(self):
        self.confusion_matrix = np.zeros((self.n_classes, self.n_classes))
        self._dev_hist = None


def dice_from_confusion(confusion) -> np.ndarray:
    """Per-class Dice of one volume from its confusion matrix: 2*h_cc / (row_c + col_c) == dc(pred == c, gt == c) (measure.py:52-99)."""
    h = np.asarray(confusion, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 * np.diag(h) / (h.sum(axis=1) + h.sum(axis=0))


def dice(result, reference) -> float:
    """2|A&B| / (|A|+|B|) on binarised inputs; NaN when both are empty."""
    a, b = np.asarray(result).astype(bool), np.asarray(reference).astype(bool)
    den = int(a.sum()) + int(b.sum())
    return float("nan") if den == 0 else 2.0 * int((a & b).sum()) / den


def _border(mask: np.ndarray, connectivity: int) -> np.ndarray:
    from scipy.ndimage import binary_erosion, generate_binary_structure
    return mask ^ binary_erosion(mask, structure=generate_binary_structure(mask.ndim, connectivity), iterations=1)


def _on_device(a, b) -> bool:
    import torch
    return torch.is_tensor(a) and torch.is_tensor(b) and a.is_cuda and b.is_cuda


def _raise_if_empty(first_empty, second_empty):
    if first_empty:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if second_empty:
        raise RuntimeError("The second supplied array does not contain any binary object.")


def _device_table(result, reference, spacing, connectivity, per_slice):
    """ops.surface_stats of two binary device objects (non-zero = inside): table [1, 2, slices or 1, 4], side 0 = result."""
    from . import ops
    if result.dim() not in (2, 3) or tuple(result.shape) != tuple(reference.shape) or (per_slice and result.dim() != 3):
        raise ValueError(f"device surface distances need two [H,W] or [D,H,W] tensors of one shape, got {tuple(result.shape)} and "
                         f"{tuple(reference.shape)}")
    vol = (-1,) + tuple(result.shape[-2:])
    return ops.surface_stats((result != 0).reshape(vol), (reference != 0).reshape(vol), 2, spacing, connectivity,
                             "2d" if (per_slice or result.dim() == 2) else "3d", foreground_only=True)


def _hd_stack_from_table(t) -> float:
    """t: host table [2, slices, 4] of one class in the per-slice form -> `hd_2D_stack`: slices with an empty mask are left out."""
    vals = [float(np.sqrt(max(t[0, z, 0], t[1, z, 0]))) for z in range(t.shape[1]) if t[0, z, 3] == 0]
    return sum(vals) / len(vals) if vals else -1


def _asd_from_table(t) -> float:
    """t: host table [2, 4] of one class in the whole-volume form -> `asd` result -> reference (side 1 = distances to the reference)."""
    return float(t[1, 1] / t[1, 2]) if t[1, 3] == 0 else 1e100


def _surface_distances_device(result, reference, voxelspacing, connectivity):
    import torch
    from . import ops
    a, b = result != 0, reference != 0
    _raise_if_empty(not bool(a.any()), not bool(b.any()))
    return torch.sqrt(ops.edt_sq(b, voxelspacing, connectivity))[ops.surface_of(a, connectivity)]


def surface_distances(result, reference, voxelspacing=None, connectivity=1) -> np.ndarray:
    """Distances from every surface voxel of `result` to the nearest surface voxel of `reference` (the surface-distance
    construction of medpy 0.4.0 `metric.binary`, carried by measure.py:1096-1128): surface = mask XOR its erosion, distances from
    the Euclidean distance transform of the reference surface's complement.  Host code (scipy), as upstream, for host inputs; two
    CUDA tensors give a device fp64 vector in the same (C) order from the HIP distance transform (ops.edt_sq / ops.surface_of)."""
    if _on_device(result, reference):
        return _surface_distances_device(result, reference, voxelspacing, connectivity)
    from scipy.ndimage import distance_transform_edt
    a, b = np.atleast_1d(np.asarray(result).astype(bool)), np.atleast_1d(np.asarray(reference).astype(bool))
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    if voxelspacing is not None:
        voxelspacing = np.ascontiguousarray(np.broadcast_to(np.asarray(voxelspacing, dtype=np.float64), (a.ndim,)))
    return distance_transform_edt(~_border(b, connectivity), sampling=voxelspacing)[_border(a, connectivity)]


def hd(result, reference, voxelspacing=None, connectivity=1) -> float:
    """Symmetric Hausdorff distance (measure.py:333-378).  Two CUDA tensors ([H,W] or [D,H,W]): one fused ops.surface_stats call."""
    if _on_device(result, reference):
        t = _device_table(result, reference, voxelspacing, connectivity, per_slice=False)[0, :, 0].cpu().numpy()
        _raise_if_empty(t[1, 2] == 0, t[0, 2] == 0)
        return float(np.sqrt(max(t[0, 0], t[1, 0])))
    return max(surface_distances(result, reference, voxelspacing, connectivity).max(),
               surface_distances(reference, result, voxelspacing, connectivity).max())


def hd_2D_stack(result, reference, pixelspacing=None, connectivity=1) -> float:
    """Mean in-plane Hausdorff distance over the slices where both masks are non-empty; -1 when there is none
    (measure.py:381-399).  Two CUDA [D,H,W] tensors: every slice and both directions in one fused ops.surface_stats call."""
    if _on_device(result, reference):
        return _hd_stack_from_table(_device_table(result, reference, pixelspacing, connectivity, per_slice=True)[0].cpu().numpy())
    vals = [hd(r, g, pixelspacing, connectivity) for r, g in zip(result, reference) if r.sum() > 0 and g.sum() > 0]
    return sum(vals) / len(vals) if vals else -1


def asd(result, reference, voxelspacing=None, connectivity=1) -> float:
    """Directed average surface distance result -> reference; 1e100 when either mask is empty (measure.py:458-548).  Two CUDA tensors
    ([H,W] or [D,H,W]): one fused ops.surface_stats call."""
    if _on_device(result, reference):
        return _asd_from_table(_device_table(result, reference, voxelspacing, connectivity, per_slice=False)[0, :, 0].cpu().numpy())
    if np.sum(result) > 0 and np.sum(reference) > 0:
        return surface_distances(result, reference, voxelspacing, connectivity).mean()
    return 1e100


def _percentile_ranks(n: int, q: float):
    """numpy's default ('linear') percentile of n sorted values sits between ranks k and min(k + 1, n - 1) at fraction g:
    v = (n - 1) * (q / 100), k = floor(v), g = v - k, all in float64.  -> (k, min(k + 1, n - 1), g)."""
    if not 0.0 <= q <= 100.0:                              # also refuses NaN
        raise ValueError("Percentiles must be in the range [0, 100]")
    v = np.float64(n - 1) * (np.float64(q) / np.float64(100.0))
    k = int(np.floor(v))
    return k, min(k + 1, n - 1), np.float64(v - np.float64(k))


def _percentile_from_ranks(a, b, g) -> float:
    """numpy's `_lerp` between the distances a (rank k) and b (rank k + 1) at fraction g: the ONE place where a percentile of surface
    distances is finished, for the host lists and for the two squared order statistics the device returns alike."""
    a, b, g = np.float64(a), np.float64(b), np.float64(g)
    d = b - a
    return float(a + d * g if g < 0.5 else b - d * (1 - g))


def _percentile_from_table(e, q: float) -> float:
    """e: one host entry (d^2 of rank k, d^2 of rank k + 1, n, flag) of ops.surface_quantiles, flag 0."""
    return _percentile_from_ranks(np.sqrt(e[0]), np.sqrt(e[1]), _percentile_ranks(int(e[2]), q)[2])


def _device_quantiles(result, reference, q, spacing, connectivity, per_slice):
    """ops.surface_quantiles (with the statistics table) of two binary device objects, read back in one copy ->
    (q entries [slices or 1, 4], statistics [2, slices or 1, 4])."""
    import torch
    from . import ops
    if result.dim() not in (2, 3) or tuple(result.shape) != tuple(reference.shape) or (per_slice and result.dim() != 3):
        raise ValueError(f"device surface distances need two [H,W] or [D,H,W] tensors of one shape, got {tuple(result.shape)} and "
                         f"{tuple(reference.shape)}")
    vol = (-1,) + tuple(result.shape[-2:])
    qt, st = ops.surface_quantiles((result != 0).reshape(vol), (reference != 0).reshape(vol), 2, (q,), spacing, connectivity,
                                   "2d" if (per_slice or result.dim() == 2) else "3d", foreground_only=True, want_stats=True)
    flat = torch.cat([qt.reshape(-1), st.reshape(-1)]).cpu().numpy()
    return flat[:qt.numel()].reshape(tuple(qt.shape))[0, :, 0], flat[qt.numel():].reshape(tuple(st.shape))[0]


def surface_distance_percentile(result, reference, q, voxelspacing=None, connectivity=1) -> float:
    """The q-th percentile (0 <= q <= 100, numpy's default linear method on float64) of the surface distances of BOTH directions pooled
    into one list: np.percentile(np.hstack((surface_distances(result, reference), surface_distances(reference, result))), q).
    q = 100 is `hd`, q = 0 the smallest pooled distance.  Two CUDA tensors ([H,W] or [D,H,W]): one ops.surface_quantiles call (exact
    rank selection on the device) and one small readback."""
    _percentile_ranks(2, q)                                # the range check, before any work
    if _on_device(result, reference):
        e, st = _device_quantiles(result, reference, q, voxelspacing, connectivity, per_slice=False)
        _raise_if_empty(st[1, 0, 2] == 0, st[0, 0, 2] == 0)
        return _percentile_from_table(e[0], q)
    pooled = np.sort(np.hstack((surface_distances(result, reference, voxelspacing, connectivity),
                                surface_distances(reference, result, voxelspacing, connectivity))))
    k, k1, g = _percentile_ranks(pooled.size, q)
    return _percentile_from_ranks(pooled[k], pooled[k1], g)


def hd95(result, reference, voxelspacing=None, connectivity=1) -> float:
    """95th-percentile Hausdorff distance as medpy >= 0.4 documents it: np.percentile(np.hstack((d(result -> reference),
    d(reference -> result))), 95).  RuntimeError on an empty mask, as `hd`."""
    return surface_distance_percentile(result, reference, 95.0, voxelspacing, connectivity)


def hd95_2D_stack(result, reference, pixelspacing=None, connectivity=1) -> float:
    """Mean in-plane `hd95` over the slices where both masks are non-empty; -1 when there is none (the form of `hd_2D_stack`,
    measure.py:381-399).  Two CUDA [D,H,W] tensors: every slice in one ops.surface_quantiles call."""
    if _on_device(result, reference):
        e, _ = _device_quantiles(result, reference, 95.0, pixelspacing, connectivity, per_slice=True)
        return _hd95_stack_from_table(e)
    vals = [hd95(r, g, pixelspacing, connectivity) for r, g in zip(result, reference) if r.sum() > 0 and g.sum() > 0]
    return sum(vals) / len(vals) if vals else -1


def _hd95_stack_from_table(e) -> float:
    """e: host entries [slices, 4] of one class in the per-slice form at q = 95 -> `hd95_2D_stack`."""
    vals = [_percentile_from_table(e[z], 95.0) for z in range(e.shape[0]) if e[z, 3] == 0]
    return sum(vals) / len(vals) if vals else -1


def assd(result, reference, voxelspacing=None, connectivity=1) -> float:
    """Average symmetric surface distance (measure.py:402-455): the mean of `asd` in both directions; 1e100 when either mask is empty,
    as `asd`.  Two CUDA tensors: both directions are rows of ONE ops.surface_stats table."""
    if _on_device(result, reference):
        return _assd_from_table(_device_table(result, reference, voxelspacing, connectivity, per_slice=False)[0, :, 0].cpu().numpy())
    return float(np.mean((asd(result, reference, voxelspacing, connectivity), asd(reference, result, voxelspacing, connectivity))))


def _assd_from_table(t) -> float:
    """t: host table [2, 4] of one class in the whole-volume form -> `assd` (side 1 = result -> reference, side 0 = the reverse)."""
    return float(np.mean((t[1, 1] / t[1, 2], t[0, 1] / t[0, 2]))) if t[1, 3] == 0 else 1e100


class runningMySegmentationScore(object):
    """Patient-wise scores of 3-D predictions (metrics.py:139-291): one row per patient, one column per (foreground class, metric).

    'Dice', 'VolError' and 'VolSim' are functions of three voxel counts per class (|pred|, |gt|, |pred & gt|); for device tensors
    those come from the confusion-matrix kernel (one launch pair and one 2*n^2-word readback per patient instead of 2*(n-1)
    full-volume host copies and masks).  The surface-distance metrics 'HD' and 'ASD' (measure.py:333-548) are, for device tensors,
    one `ops.surface_stats` call each (exact fp64 distance transform of every class and both directions in 4 / 5 launches) and one
    readback of their small tables per patient: no label volume leaves the device.  numpy inputs run scipy on the host, as upstream.
    'HD95' (`hd95_2D_stack`, with the conventions of 'HD') and 'ASSD' (`assd`, with those of 'ASD') are this project's additions to the
    table: 'HD95' comes from `ops.surface_quantiles`, in the same launches as 'HD' when both are asked for, 'ASSD' from the table of
    'ASD'.
    'ECE', 'NLL', 'Brier' and 'Entropy' (also additions) are PATIENT-level columns, named exactly so and appended after the per-class
    columns: expected calibration error over `calibration_bins` equal-width confidence bins, mean negative log-likelihood (nats), mean
    Brier score and mean predictive entropy (bits) of the logits handed to `update` (uncertainty.py).  Device logits: one
    `ops.predictive_stats` call whose two small tables join the voxel counts' readback; numpy logits: the float64 host statement."""
    SUPPORTED = ("Dice", "VolError", "VolSim", "HD", "ASD", "HD95", "ASSD")      # one column per foreground class
    PATIENT_LEVEL = ("ECE", "NLL", "Brier", "Entropy")                          # one column per patient, accepted in metrics_list as well

    def __init__(self, n_classes, idx2cls_dict=None, metrics_list=("Dice",), foreground_only=False, calibration_bins=15):
        self.n_classes, self.metrics, self.foreground_only = n_classes, list(metrics_list), foreground_only
        if idx2cls_dict is None:
            idx2cls_dict = {1: "foreground"} if foreground_only else {c: str(c) for c in range(n_classes)}
        self.idx2cls_dict = idx2cls_dict
        self.multi_scores, self.tables, self.header = {}, [], ["patient_id"]
        for m in self.metrics:
            if m not in self.SUPPORTED + self.PATIENT_LEVEL:
                raise NotImplementedError(f"metric {m!r}: only {self.SUPPORTED + self.PATIENT_LEVEL} are computed by this build")
        self.calibration_bins = int(calibration_bins)
        self.patient_metrics = [m for m in self.metrics if m in self.PATIENT_LEVEL]
        self.metrics = [m for m in self.metrics if m not in self.PATIENT_LEVEL]
        for c, name in idx2cls_dict.items():
            if c > 0:
                for m in self.metrics:
                    self.multi_scores[name + "_" + m] = []
                    self.header.append(name + "_" + m)
        for m in self.patient_metrics:
            self.multi_scores[m] = []
            self.header.append(m)

    def _counts(self, preds, gts, extra=None):
        """-> (pred_count[c], gt_count[c], intersection[c]) as the reference's per-class binarisation counts them
        (metrics.py:205-223): a ground-truth label outside [0, n) belongs to no class, the predicted voxel under it still counts.
        extra: flat int64 device tensors that ride along in the device branch's readback; their host copy is left in self._readback."""
        import torch
        n = self.n_classes
        self._readback = None
        if torch.is_tensor(preds) and torch.is_tensor(gts) and preds.is_cuda and gts.is_cuda:
            from . import ops
            both = torch.stack([ops.confusion_hist(gts, preds, n), ops.confusion_hist(preds, preds, n)])
            if extra:
                flat = torch.cat([both.reshape(-1)] + list(extra)).cpu().numpy()
                both, self._readback = flat[:2 * n * n].reshape(2, n, n), flat[2 * n * n:]
            else:
                both = both.cpu().numpy()
            h, hp = both[0], both[1]
            if self.foreground_only and int(h.sum()) != gts.numel():
                raise ValueError("foreground_only with labels outside [0, n_classes): pass host arrays")
            pc, gc, ic = np.diag(hp).copy(), h.sum(axis=1), np.diag(h).copy()
        else:
            p, g = np.asarray(preds).reshape(-1).astype(np.int64), np.asarray(gts).reshape(-1).astype(np.int64)
            if self.foreground_only:                       # gt > 0 / pred > 0 (any positive label is foreground upstream)
                p, g = (p > 0).astype(np.int64), (g > 0).astype(np.int64)
            pc = np.bincount(p[(p >= 0) & (p < n)], minlength=n)
            gc = np.bincount(g[(g >= 0) & (g < n)], minlength=n)
            same = p[(p == g) & (p >= 0) & (p < n)]
            ic = np.bincount(same, minlength=n)
            return pc, gc, ic
        if self.foreground_only:                           # everything that is not background, on both sides
            fg_i = h[1:, 1:].sum()
            pc, gc, ic = np.array([0, pc[1:].sum()]), np.array([0, gc[1:].sum()]), np.array([0, fg_i])
        return pc, gc, ic

    def _surface_tables(self, preds, gts, surf, voxel_spacing):
        """{'HD': host table [classes, 2, slices, 4], 'ASD': [classes, 2, 1, 4], 'HD95': [classes, slices, 1, 4]} of one patient from
        ops.surface_stats / ops.surface_quantiles (same masks, 8- / 18-neighbourhood surfaces and spacing convention as the host branch
        of `update`); all tables come back in one copy.  'HD' with 'HD95' is ONE surface_quantiles call that also writes the statistics
        table (3 launches more than surface_stats alone, against a second full set of distance passes); 'ASSD' reads the 'ASD' table."""
        import torch
        from . import ops
        if any(c >= self.n_classes for c in self.idx2cls_dict):
            raise ValueError("idx2cls_dict names a class outside [0, n_classes): pass host arrays")
        tabs = {}
        if "HD95" in surf and "HD" in surf:
            tabs["HD95"], tabs["HD"] = ops.surface_quantiles(preds, gts, self.n_classes, (95.0,), voxel_spacing[:2], 2, "2d",
                                                             self.foreground_only, want_stats=True)
        elif "HD95" in surf:
            tabs["HD95"] = ops.surface_quantiles(preds, gts, self.n_classes, (95.0,), voxel_spacing[:2], 2, "2d", self.foreground_only)
        elif "HD" in surf:
            tabs["HD"] = ops.surface_stats(preds, gts, self.n_classes, voxel_spacing[:2], 2, "2d", self.foreground_only)
        if "ASD" in surf or "ASSD" in surf:
            tabs["ASD"] = ops.surface_stats(preds, gts, self.n_classes, voxel_spacing, 2, "3d", self.foreground_only)
        flat = torch.cat([t.reshape(-1) for t in tabs.values()]).cpu().numpy()
        out, lo = {}, 0
        for k, t in tabs.items():
            out[k] = flat[lo:lo + t.numel()].reshape(tuple(t.shape))
            lo += t.numel()
        return out

    def calibration_tables(self, logits, gts, members=1):
        """The (stats, bins) tables of one chunk of slices (uncertainty.py): logits [members * n, C, H, W], gts [n, H, W].  Device logits
        -> ops.PredictiveStats with device tables (2 launches, nothing read back); numpy logits -> the float64 host statement.  The
        tables are per slice, so the chunks of a patient concatenate: `update(logits=[...])` takes a list of these."""
        import torch
        if torch.is_tensor(logits) and logits.is_cuda:
            from . import ops
            label = torch.as_tensor(gts).to(device=logits.device, dtype=torch.int64).contiguous()
            return ops.predictive_stats(logits.float(), label, members=members, n_bins=self.calibration_bins, want=())
        from . import uncertainty
        host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)      # noqa: E731
        return uncertainty.predictive_stats_host(host(logits), host(gts), members=members, n_bins=self.calibration_bins)

    def _calibration(self, logits, gts, members):
        """-> (chunk tables, flat int64 device tensors for the joined readback): `logits` is one array / tensor of the whole volume, or a
        list of chunks along the slice axis, each an array / tensor or the result of `calibration_tables`."""
        import torch
        chunks, lo, tabs = (list(logits) if isinstance(logits, (list, tuple)) and not hasattr(logits, "stats") else [logits]), 0, []
        for ch in chunks:
            if not hasattr(ch, "stats"):
                n = int(ch.shape[0]) // int(members)
                ch = self.calibration_tables(ch, gts[lo:lo + n], members)
            lo += int(ch.stats.shape[0])
            tabs.append(ch)
        if lo != int(gts.shape[0]):
            raise ValueError(f"the logits cover {lo} slices, the volume has {int(gts.shape[0])}")
        on_device = [torch.is_tensor(t.stats) for t in tabs]
        if any(on_device) and not all(on_device):
            raise ValueError("the chunks of one patient's logits must all be on the device or all on the host")
        extra = [q for t in tabs for q in (t.stats.reshape(-1).view(torch.int64), t.bins.reshape(-1))] if all(on_device) else []
        return tabs, extra      # (fp64 bits ride as int64)

    def _calibration_scores(self, tabs, extra, readback, pixels):
        """the four columns from the chunk tables; `readback`: the host copy of `extra` when it rode along with the voxel counts"""
        from . import uncertainty
        import torch
        if extra:
            flat = readback if readback is not None else torch.cat(extra).cpu().numpy()
            stats, bins, lo = [], [], 0
            for t in tabs:
                ns, nb = t.stats.numel(), t.bins.numel()
                stats.append(flat[lo:lo + ns].view(np.float64).reshape(-1, 6))
                bins.append(flat[lo + ns:lo + ns + nb].reshape(tuple(t.bins.shape)))
                lo += ns + nb
        else:
            stats, bins = [np.asarray(t.stats) for t in tabs], [np.asarray(t.bins) for t in tabs]
        return uncertainty.calibration_from_tables(np.concatenate(stats), np.concatenate(bins), pixels=pixels)

    def update(self, pid, preds, gts, voxel_spacing=None, logits=None, members=1):
        """preds / gts: integer volumes [n_slices, H, W] (numpy, or both torch tensors on the GPU); returns the patient's row.
        logits (for 'ECE' / 'NLL' / 'Brier' / 'Entropy'): the volume's logits [members * n_slices, C, H, W], member-major, on the device
        or as numpy, or a list of chunks along the slice axis (see `calibration_tables`)."""
        if tuple(preds.shape) != tuple(gts.shape):
            raise AssertionError(f"pid :{pid} shape not consistent: pred {tuple(preds.shape)} vs gt {tuple(gts.shape)}")
        if voxel_spacing is not None and len(voxel_spacing) != 3:
            raise AssertionError(f"check voxel spacing, {voxel_spacing}")
        cal_tabs, extra = None, None
        if self.patient_metrics:
            if logits is None:
                raise ValueError(f"{self.patient_metrics} need the logits of the volume: update(..., logits=, members=)")
            cal_tabs, extra = self._calibration(logits, gts, members)
        pc, gc, ic = self._counts(preds, gts, extra)
        surf = [m for m in self.metrics if m in ("HD", "ASD", "HD95", "ASSD")]
        if surf:
            if voxel_spacing is None:
                raise ValueError("'HD' / 'ASD' / 'HD95' / 'ASSD' need the voxel spacing (x, y, z) of the volume")
            if "HD" in surf or "HD95" in surf:      # metrics.py:225-229: the in-plane pair is voxel_spacing[:2]; upstream's own guard on the axis order
                assert voxel_spacing[0] >= voxel_spacing[2], "z spacing should be in last dim in the cardiac imaging"
            if _on_device(preds, gts):                     # one fused launch sequence per metric, ONE readback of the small tables
                dev_tab = self._surface_tables(preds, gts, surf, voxel_spacing)
            else:
                dev_tab = None
                p_h = preds.detach().cpu().numpy() if hasattr(preds, "detach") else np.asarray(preds)
                g_h = gts.detach().cpu().numpy() if hasattr(gts, "detach") else np.asarray(gts)
        row = [str(pid)]
        for c, name in self.idx2cls_dict.items():
            if c == 0:
                continue
            v1, v2, inter = int(pc[c]), int(gc[c]), int(ic[c])
            for m in self.metrics:
                if m == "Dice":                            # medpy dc: ZeroDivisionError -> 0.0
                    score = 2.0 * inter / float(v1 + v2) if v1 + v2 else 0.0
                elif m in ("HD", "ASD") and dev_tab is not None:
                    t = dev_tab[m][0 if self.foreground_only else c - 1]
                    score = float(_hd_stack_from_table(t) if m == "HD" else _asd_from_table(t[:, 0]))
                elif m in ("HD95", "ASSD") and dev_tab is not None:
                    ci = 0 if self.foreground_only else c - 1
                    score = float(_hd95_stack_from_table(dev_tab["HD95"][ci][:, 0]) if m == "HD95" else _assd_from_table(dev_tab["ASD"][ci][:, 0]))
                elif m in ("HD", "ASD", "HD95", "ASSD"):
                    pm = (p_h > 0) if self.foreground_only else (p_h == c)
                    gm = (g_h > 0) if self.foreground_only else (g_h == c)
                    if m == "HD":                          # 2-D stack, 8-neighbourhood surfaces (metrics.py:224-230)
                        score = hd_2D_stack(pm, gm, pixelspacing=voxel_spacing[:2], connectivity=2)
                    elif m == "HD95":                      # the same conventions as 'HD'
                        score = hd95_2D_stack(pm, gm, pixelspacing=voxel_spacing[:2], connectivity=2)
                    elif m == "ASSD":                      # the same conventions as 'ASD'
                        score = assd(pm, gm, voxelspacing=voxel_spacing, connectivity=2)
                    else:
                        score = asd(pm, gm, voxelspacing=voxel_spacing, connectivity=2)
                    score = float(score)
                elif m == "VolError":                      # (pred - gt) / gt, numpy float division (inf / nan on an empty gt)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        score = float(np.float64(v1 - v2) / np.float64(1.0 * v2))
                else:                                      # VolSim, measure.py:668-722
                    if v2 == 0:
                        raise RuntimeError("The second supplied array does not contain any binary object.")
                    score = float(1 - np.abs(v1 - v2) / np.abs(float(v2 + v1)))
                self.multi_scores[name + "_" + m].append(score)
                row.append(score)
        if cal_tabs is not None:
            cal = self._calibration_scores(cal_tabs, extra, self._readback, int(np.prod(tuple(gts.shape))))
            for m in self.patient_metrics:
                self.multi_scores[m].append(cal[m])
                row.append(cal[m])
        self.tables.append(row)
        return row

    def get_scores(self, save_path=None):
        """-> ({col_mean, col_std}, [[means as '%.3f'], [stds]], header); written as csv when save_path is given."""
        summary, rows, header = {}, [[], []], []
        for k, vals in self.multi_scores.items():
            mean, std = np.mean(vals), np.std(vals)
            summary[k + "_mean"], summary[k + "_std"] = mean, std
            rows[0].append("{:.3f}".format(mean))
            rows[1].append("{:.3f}".format(std))
            header.append(k)
        if save_path is not None:
            import pandas as pd
            pd.DataFrame(rows, columns=header).to_csv(save_path, index=False)
        return summary, rows, header

    def save_patient_wise_result_to_csv(self, save_path):
        import pandas as pd
        df = pd.DataFrame(self.tables, columns=self.header)
        if save_path is not None:
            df.to_csv(save_path, index=False)
        return df

    def reset(self):
        for k in self.multi_scores:
            self.multi_scores[k] = []
        self.tables = []
