"""Host restatement of the counter-hash RNG of csrc/ctl_mask.hip and csrc/ctl_io.hip: plain 64-bit integer arithmetic on numpy.uint64
(wrap-around), nothing imported from the package.  Test infrastructure only.

    splitmix_out(seed, idx)    output number idx + 1 of splitmix64 seeded with `seed` (idx = 0 is the first output)
    hash_uniform(seed, idx)    its top 24 bits as a float32 in [0, 1)                         (dropout keep draws, ctl_uniform)
    state_seed(s0, s1, salt)   seed of one call site of one training step from the device state [seed, step, ...]
    io_mix(z)                  one splitmix64 step on z (the finaliser ctl_noise_clamp keys with seed ^ io_mix(index))
    box_muller_uniforms        the two 24-bit uniforms of ctl_noise_clamp's device noise: u1 in (0, 1], u2 in [0, 1)
    normal_f64                 sigma * sqrt(-2 ln u1) * cos(2 pi u2) in float64
"""
import numpy as np

U64 = np.uint64
GOLDEN = U64(0x9E3779B97F4A7C15)
M1 = U64(0xBF58476D1CE4E5B9)
M2 = U64(0x94D049BB133111EB)
STEP_MUL = U64(0xD1B54A32D192ED03)
MASK64 = (1 << 64) - 1


def u64(v):
    """Python ints (any sign, any size) or integer arrays -> numpy.uint64 modulo 2^64"""
    if isinstance(v, (int, np.integer)):
        return U64(int(v) & MASK64)
    a = np.asarray(v)
    if a.dtype == np.uint64:
        return a
    if a.dtype.kind == "i":
        return a.astype(np.int64).view(np.uint64)
    if a.dtype.kind == "u":
        return a.astype(np.uint64)
    return np.array([int(x) & MASK64 for x in a.ravel()], dtype=np.uint64).reshape(a.shape)


def _finalise(z):
    z = (z ^ (z >> U64(30))) * M1
    z = (z ^ (z >> U64(27))) * M2
    return z ^ (z >> U64(31))


def splitmix_out(seed, idx):
    with np.errstate(over="ignore"):
        return _finalise(u64(seed) + (u64(idx) + U64(1)) * GOLDEN)


def hash_uniform(seed, idx):
    top = (splitmix_out(seed, idx) >> U64(40)).astype(np.float32)          # < 2^24: exact
    return top * np.float32(1.0 / 16777216.0)


def state_seed(state0, state1, salt):
    with np.errstate(over="ignore"):
        z = u64(state0) + (u64(state1) + U64(1)) * STEP_MUL + u64(salt) * GOLDEN
        z = (z ^ (z >> U64(32))) * M1
        return z ^ (z >> U64(29))


def io_mix(z):
    with np.errstate(over="ignore"):
        return _finalise(u64(z) + GOLDEN)


def box_muller_uniforms(seed, idx):
    h = io_mix(u64(seed) ^ io_mix(idx))
    u1 = ((h >> U64(40)) + U64(1)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    u2 = ((h >> U64(8)) & U64(0xFFFFFF)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u1, u2


def normal_f64(seed, idx, sigma):
    """(value, radius, cosine): sigma * radius * cosine with radius = sqrt(-2 ln u1), cosine = cos(2 pi u2), all float64"""
    u1, u2 = box_muller_uniforms(seed, idx)
    radius = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    cosine = np.cos(2.0 * np.pi * u2.astype(np.float64))
    return float(sigma) * radius * cosine, radius, cosine
