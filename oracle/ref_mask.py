"""Host restatement of the latent-mask generator tail and of dropout2d (csrc/ctl_mask.hip), numpy only, nothing imported from the
package.  Test infrastructure only.  Arrays are [n, hw, c] (the kernels' NHWC memory); score / mask rows are [n, L] with L = c in
channel mode (mode 0) and L = hw in spatial mode (mode 1).

    score(grad, mode)                 signed mean over hw (mode 0) or over c (mode 1) in float64
    score_exact_f32(grad, mode)       for integer-valued gradients: fp32(sum) * fp32(1 / count), the only value an fp32 kernel can give
    select(score, k, soft_noise)      threshold = sort(descending)[k]; hit = score > threshold; mask = 0.5 * noise | 0 where hit, else 1
    select_by_count(...)              the same selection written as  #{j : s_j >= s_i} <= k
    apply(code, mask, mode)           code * mask, the mask broadcast over hw (mode 0) or over c (mode 1), one fp32 multiply
    dropout2d(z, keep, p, ...)        z * (keep * fp32(1 / (1 - p))) with one rounding to bf16 where stored as bf16, and upstream's
                                      full-size mask  out == z
"""
import numpy as np

F32 = np.float32


def score(grad, mode):
    g = np.asarray(grad, dtype=np.float64)
    return g.mean(axis=1) if mode == 0 else g.mean(axis=2)


def score_exact_f32(grad, mode):
    """Integer-valued grad with |sum| < 2^24: every partial sum is exact in fp32 in any order, so the score is one rounded product"""
    g = np.asarray(grad, dtype=np.float64)
    axis = 1 if mode == 0 else 2
    s = g.sum(axis=axis)
    assert np.array_equal(g, np.rint(g)) and np.abs(g).sum(axis=axis).max() < 2 ** 24
    inv = F32(1.0) / F32(g.shape[axis])
    return s.astype(F32) * inv


def clamp_k(k, L):
    return min(max(int(k), 0), L - 1)


def _mask_values(hit, soft_noise):
    if soft_noise is None:
        return np.where(hit, F32(0.0), F32(1.0)).astype(F32)
    return np.where(hit, F32(0.5) * np.asarray(soft_noise, dtype=F32), F32(1.0)).astype(F32)


def select(score_rows, k, soft_noise=None):
    s = np.asarray(score_rows)
    thr = -np.sort(-s, axis=1, kind="stable")[:, k][:, None]          # descending; -x is exact, +0 / -0 compare equal either way
    return _mask_values(s > thr, soft_noise)


def select_by_count(score_rows, k, soft_noise=None):
    """entry i is hit  <=>  fewer than k + 1 entries of its row are >= it (written without a sort: a searchsorted count per entry)"""
    s = np.asarray(score_rows)
    hit = np.empty(s.shape, dtype=bool)
    for r in range(s.shape[0]):
        asc = np.sort(s[r] + 0.0)                                      # (+ 0.0 turns -0 into +0: the count compares values, not bits)
        ge = s.shape[1] - np.searchsorted(asc, s[r] + 0.0, side="left")
        hit[r] = ge <= k
    return _mask_values(hit, soft_noise)


def apply(code, mask, mode):
    c = np.asarray(code, dtype=F32)
    m = np.asarray(mask, dtype=F32)
    with np.errstate(invalid="ignore"):
        return c * (m[:, None, :] if mode == 0 else m[:, :, None])


def to_bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; finite inputs and infinities"""
    u = np.asarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    u = u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))
    return (u >> np.uint64(16)).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def dropout2d(z, keep, p, bf16_in=False, bf16_out=False):
    """z [n, hw, c] (fp32 values; bf16_in: already bf16-representable), keep [n, c] of {0, 1}.  Returns (out, mask_full): out as fp32
    values, or as bf16 bit patterns (uint16) with bf16_out; mask_full = 1 where out == z (the fp32 form only, else None)"""
    z = np.asarray(z, dtype=F32)
    if bf16_in:
        assert np.array_equal(from_bf16_bits(to_bf16_bits(z)), z)
    inv = F32(1.0) / (F32(1.0) - F32(p))
    mult = np.asarray(keep, dtype=F32) * inv
    out = z * mult[:, None, :]
    if bf16_out:
        return to_bf16_bits(out), None
    return out, (None if bf16_in else (out == z).astype(F32))
