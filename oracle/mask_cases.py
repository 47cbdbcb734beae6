"""Shapes, tie fixtures and rank choices shared by tests/test_ref_mask_rng_io_cpu.py and tests/test_mask_exact_gpu.py, numpy only.

A fixture is first a table of integer score SUMS T[n, L]; `grads_for` then spreads each sum over the `count` gradients it is the sum
of (hw in channel mode, c in spatial mode) as integers in [-3, 3] in a random order, so every partial sum is exact in fp32 whatever
the order and the device score must be fp32(T) * fp32(1 / count) bit for bit.  Distinct sums give distinct scores (|T| < 2^15, so two
sums differ by more than 2^-15 relative, far above the 2^-24 of the one rounding).

    all_equal     every score of a row equal                        nothing may be masked, for any k
    one_nonzero   all zero except one entry
    half_dead     half the row zero (dead channels), half distinct  (as distinct as [-3 count, 3 count] allows: c = 4 gives 24 values)
    pairs         every value twice                                 k chosen with sort[k] == sort[k-1], and with sort[k] == sort[k+1]
    signed_zero   gradients mixing +0.0 and -0.0 among a few others (the sums come out +0; score rows that really mix +0 and -0 are
                  built by `signed_zero_scores` and go to the apply call, which takes scores as they are)
    random        random integer sums, k placed where sort[k-1] != sort[k] (no tie at rank k: exactly k entries are masked)
"""
import zlib

import numpy as np

F32 = np.float32

# (n, c, h, w): the smallest shapes that reach each branch of the launch selection in csrc/ctl_mask.hip
SHAPES = [
    (1, 4, 1, 1),          # smallest shape
    (3, 8, 3, 3),          # small ragged shape
    (2, 128, 16, 16),      # configured size
    (9, 16, 8, 8),         # 8 blocks per image on one XCD each, grid rounded up to 16 images with 7 idle
    (70, 8, 4, 4),         # one block per image, many images
    (1, 256, 16, 16),      # hw * c = 65536 exactly, widest c, rolled score loop
    (1, 64, 32, 32),       # spatial L = 1024 exactly, the widest one-launch instantiation
    (1, 64, 33, 32),       # just over both limits: split sums + finalising apply (channel), bitonic threshold with L = 1056 (spatial)
    (2, 128, 32, 32),      # streaming path, spatial L = 1024 ranked in the apply kernel
    (1, 4, 41, 25),        # L = 1025
    (3, 32, 48, 40),       # L = 1920, not a power of two
    (2, 4, 64, 128),       # L = 8192, the maximum
]
FIXTURES = ("all_equal", "one_nonzero", "half_dead", "pairs", "signed_zero", "random")
MIN_LEN = {"all_equal": 1, "one_nonzero": 2, "half_dead": 4, "pairs": 4, "signed_zero": 2, "random": 2}


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def row_len(shape, mode):
    n, c, h, w = shape
    return c if mode == 0 else h * w


def summands(shape, mode):
    n, c, h, w = shape
    return h * w if mode == 0 else c


def _shuffle_rows(t, rng):
    return np.take_along_axis(t, np.argsort(rng.random(t.shape), axis=1), axis=1)


def target_sums(fixture, n, L, count, rng):
    B = 3 * count
    if fixture == "all_equal":
        return np.repeat(((np.arange(n) + 1) % (2 * B + 1) - B)[:, None], L, axis=1).astype(np.int64)
    if fixture == "one_nonzero":
        t = np.zeros((n, L), dtype=np.int64)
        t[np.arange(n), rng.integers(0, L, n)] = np.where(np.arange(n) % 2 == 0, min(3, B), -min(3, B))
        return t
    if fixture == "half_dead":
        nonzero = rng.permutation(np.concatenate([np.arange(-B, 0), np.arange(1, B + 1)]))
        row = np.concatenate([np.zeros(L - L // 2, dtype=np.int64), nonzero[np.arange(L // 2) % (2 * B)]])
        return _shuffle_rows(np.repeat(row[None], n, axis=0), rng)
    if fixture == "pairs":
        vals = rng.permutation(np.arange(-B, B + 1))
        row = vals[(np.arange(L) // 2) % (2 * B + 1)]
        return _shuffle_rows(np.repeat(row[None], n, axis=0), rng)
    if fixture == "signed_zero":
        m = min(2, B)
        return np.where(rng.random((n, L)) < 0.25, rng.integers(-m, m + 1, (n, L)), 0).astype(np.int64)
    if fixture == "random":
        return rng.integers(-B, B + 1, (n, L)).astype(np.int64)
    raise ValueError(fixture)


def grads_for(T, count, mode, rng, signed_zero=False):
    """float32 [n, hw, c] of integers in [-3, 3] whose sums over hw (mode 0) or over c (mode 1) are T[n, L]"""
    n, L = T.shape
    a = np.abs(T)
    assert a.max() <= 3 * count
    j = np.arange(count)[None, None, :]
    v = np.where(j < (a // 3)[..., None], 3, np.where(j == (a // 3)[..., None], (a % 3)[..., None], 0)) * np.sign(T)[..., None]
    v = v.astype(np.int64)
    if count > 1:
        for _ in range(6):          # zero-sum +1 / -1 moves between two slots: other values than 0 and +-3, same sum
            p, q = rng.integers(0, count, (n, L, 1)), rng.integers(0, count, (n, L, 1))
            vp, vq = np.take_along_axis(v, p, 2), np.take_along_axis(v, q, 2)
            ok = (p != q) & (vp <= 2) & (vq >= -2)
            np.put_along_axis(v, p, vp + ok, 2)
            np.put_along_axis(v, q, np.take_along_axis(v, q, 2) - ok, 2)
        v = np.take_along_axis(v, np.argsort(rng.random(v.shape), axis=2), axis=2)
    assert np.array_equal(v.sum(axis=2), T) and np.abs(v).max() <= 3
    g = v.astype(F32)
    if signed_zero:
        g = np.where((g == 0) & (rng.random(g.shape) < 0.5), F32(-0.0), g)
    return np.ascontiguousarray(g.transpose(0, 2, 1) if mode == 0 else g)


def signed_zero_scores(n, L, rng):
    """score rows mixing +0.0 and -0.0 (they compare equal) with a few entries above and below"""
    s = np.where(rng.random((n, L)) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    other = rng.random((n, L)) < 0.2
    return np.where(other, rng.integers(-2, 3, (n, L)).astype(F32) * F32(0.25), s).astype(F32)


def base_ks(L):
    return sorted({k for k in (0, 1, L // 2, L - 2, L - 1) if 0 <= k < L})


def device_k_in_range(L):
    return L // 3            # the one k of each shape that is passed through a device int32


def device_ks_outside(L):
    return (-5, L + 7)       # clamped to [0, L - 1] by the kernels


def special_ks(fixture, score_rows):
    """ranks that the fixture is about, from row 0 sorted descending"""
    s = -np.sort(-np.asarray(score_rows)[0])
    L = s.size
    mid, out = L // 2, []
    order = sorted(range(1, L), key=lambda k: abs(k - mid))
    if fixture == "pairs":
        prev = [k for k in order if s[k] == s[k - 1]]
        nxt = [k for k in sorted(range(0, L - 1), key=lambda k: abs(k - mid)) if s[k] == s[k + 1] and (k == 0 or s[k - 1] != s[k])]
        out = prev[:1] + nxt[:1]
    if fixture == "random":
        out = [k for k in order if s[k] != s[k - 1]][:1]
    return out


def all_ks(fixture, score_rows):
    L = np.asarray(score_rows).shape[1]
    return sorted(set(base_ks(L)) | set(special_ks(fixture, score_rows)) | {device_k_in_range(L)})


def code_for(shape, rng):
    """random fp32 [n, hw, c] with a few +-0.0, +-inf and denormals"""
    n, c, h, w = shape
    code = rng.standard_normal((n, h * w, c)).astype(F32)
    flat = code.reshape(-1)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-41, 1.4e-45], dtype=F32)
    pos = rng.permutation(flat.size)[:min(flat.size // 2, 2 * special.size)]
    flat[pos] = special[np.arange(pos.size) % special.size]
    return code


def fixtures_for(shape, mode):
    """yields (fixture, grad [n,hw,c] float32, T [n,L]) for every fixture the row length allows"""
    n, c, h, w = shape
    L, count = row_len(shape, mode), summands(shape, mode)
    for fx in FIXTURES:
        if L < MIN_LEN[fx]:
            continue
        rng = rng_for(shape, mode, fx)
        T = target_sums(fx, n, L, count, rng)
        yield fx, grads_for(T, count, mode, rng, signed_zero=(fx == "signed_zero")), T
