"""Host restatement of the I/O kernels of csrc/ctl_io.hip from their header contract (include/ctl_hip.h), numpy only, nothing imported
from the package.  Test infrastructure only.

    confusion(label_true, label_pred, n_class)   hist[n_class * t + p] counts, elements with t outside [0, n) or p >= n ignored
    rescale(x, new_min, new_max, eps)            per plane ((x - mn) / ((mx - mn) + eps)) * (new_max - new_min) + new_min, float32,
                                                 one rounding per operation, in exactly this order
    noise_clamp(x, noise, lo, hi)                min(max(x + noise, lo), hi) in float32
    crop_or_pad(src, new_h, new_w)               dst[y][x] = src[y + floor((h - new_h) / 2)][x + floor((w - new_w) / 2)] or 0 outside
"""
import numpy as np

F32 = np.float32


def confusion(label_true, label_pred, n_class, hist=None):
    t = np.asarray(label_true).astype(np.int64).ravel()
    p = np.asarray(label_pred).astype(np.int64).ravel()
    ok = (t >= 0) & (t < n_class) & (p >= 0) & (p < n_class)
    h = np.bincount(n_class * t[ok] + p[ok], minlength=n_class * n_class).astype(np.int64).reshape(n_class, n_class)
    return h if hist is None else np.asarray(hist, dtype=np.int64).reshape(n_class, n_class) + h


def rescale(x, new_min=0.0, new_max=1.0, eps=1e-20):
    """x [planes, plane_elems] float32 without NaN"""
    x = np.asarray(x, dtype=F32)
    assert x.ndim == 2 and not np.isnan(x).any()
    mn = x.min(axis=1, keepdims=True)
    mx = x.max(axis=1, keepdims=True)
    rng = F32(new_max) - F32(new_min)
    den = (mx - mn) + F32(eps)
    with np.errstate(all="ignore"):
        return ((x - mn) / den) * rng + F32(new_min)


def noise_clamp(x, noise, lo=0.0, hi=1.0):
    s = np.asarray(x, dtype=F32) + np.asarray(noise, dtype=F32)
    return np.minimum(np.maximum(s, F32(lo)), F32(hi))


def crop_or_pad(src, new_h, new_w):
    """src [n, h, w] of any dtype"""
    src = np.asarray(src)
    n, h, w = src.shape
    hs = (h - new_h) // 2          # Python's // is the floor, also of a negative half-difference
    ws = (w - new_w) // 2
    dst = np.zeros((n, new_h, new_w), dtype=src.dtype)
    sy, sx = np.arange(new_h) + hs, np.arange(new_w) + ws
    oky, okx = (sy >= 0) & (sy < h), (sx >= 0) & (sx < w)
    b = np.arange(n)
    dst[np.ix_(b, np.flatnonzero(oky), np.flatnonzero(okx))] = src[np.ix_(b, sy[oky], sx[okx])]
    return dst
