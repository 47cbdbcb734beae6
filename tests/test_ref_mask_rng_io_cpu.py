"""The host references of oracle/ref_rng.py, ref_mask.py and ref_io.py, which tests/test_mask_exact_gpu.py, test_rng_exact_gpu.py and
test_io_exact_gpu.py hold the HIP kernels to, checked on the CPU: published splitmix64 outputs, the two selection forms against each
other and against the oracle's statement of model_util.py:231-244 (oracle/ref_cpu.py::rank_select_mask, on CPU tensors), the
upstream-recorded results of tests/golden/io_cases.pt, and the cap on the number of masked entries for every tie fixture."""
import os

import numpy as np
import pytest
import torch

from oracle import mask_cases as MC
from oracle import ref_cpu, ref_io, ref_mask, ref_rng

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M64 = (1 << 64) - 1


# ================================================================================================ RNG
def _splitmix_py(seed, idx):
    """Python integers only: output number idx + 1 of splitmix64"""
    z = (seed + (idx + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_splitmix_known_answers():
    out = ref_rng.splitmix_out(0, np.arange(3, dtype=np.uint64))
    assert [int(v) for v in out] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = ref_rng.hash_uniform(0, np.arange(3, dtype=np.uint64))
    assert u.dtype == np.float32
    assert [float(v) for v in u] == [0.8833107948303223, 0.4315279722213745, 0.02643376588821411]
    assert [float(v) for v in u] == [(x >> 40) / 2.0 ** 24 for x in (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)]


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63, 2 ** 64 - 1, 0x0123456789ABCDEF])
def test_rng_wraps_like_64_bit_integers(seed):
    idx = np.array([0, 1, 255, 256, 2 ** 31, 2 ** 32 + 5, 2 ** 63 - 1], dtype=np.uint64)
    out = ref_rng.splitmix_out(seed, idx)
    assert [int(v) for v in out] == [_splitmix_py(seed, int(i)) for i in idx]
    u = ref_rng.hash_uniform(seed, idx)
    assert [float(v) for v in u] == [(_splitmix_py(seed, int(i)) >> 40) / 2.0 ** 24 for i in idx]
    assert (u >= 0).all() and (u < 1).all()
    # a seed given as the int64 the device state holds is the same seed
    signed = seed - (1 << 64) if seed >= 1 << 63 else seed
    assert np.array_equal(ref_rng.splitmix_out(np.array([signed], dtype=np.int64), idx[:1]), out[:1])
    assert int(ref_rng.io_mix(seed)) == _splitmix_py(seed, 0)


@pytest.mark.parametrize("s0,s1,salt", [(0, 0, 0), (1234, 7, 1), (2 ** 63, 2 ** 40, 2 ** 32 + 5), (2 ** 64 - 1, 2 ** 63 - 1, 2 ** 64 - 1)])
def test_state_seed_and_box_muller_uniforms(s0, s1, salt):
    z = (s0 + (s1 + 1) * 0xD1B54A32D192ED03 + salt * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 32)) * 0xBF58476D1CE4E5B9) & M64
    assert int(ref_rng.state_seed(s0, s1, salt)) == z ^ (z >> 29)
    idx = np.array([0, 1, 2 ** 20 + 3], dtype=np.uint64)
    u1, u2 = ref_rng.box_muller_uniforms(s0, idx)
    for i, a, b in zip(idx, u1, u2):
        h = _splitmix_py(s0 ^ _splitmix_py(int(i), 0), 0)
        assert float(a) == ((h >> 40) + 1) / 2.0 ** 24 and float(b) == ((h >> 8) & 0xFFFFFF) / 2.0 ** 24
    assert (u1 > 0).all() and (u1 <= 1).all() and (u2 >= 0).all() and (u2 < 1).all()
    val, radius, cosine = ref_rng.normal_f64(s0, idx, 0.05)
    assert np.allclose(val, 0.05 * np.sqrt(-2 * np.log(u1.astype(np.float64))) * np.cos(2 * np.pi * u2.astype(np.float64)), rtol=1e-15, atol=0)
    assert radius.max() <= np.sqrt(2 * 24 * np.log(2)) and np.abs(cosine).max() <= 1


# ================================================================================================ selection
def _fixture_scores(shape, mode):
    for fx, grad, T in MC.fixtures_for(shape, mode):
        yield fx, ref_mask.score_exact_f32(grad, mode), T
    L = MC.row_len(shape, mode)
    if L >= 2:
        yield "signed_zero_scores", MC.signed_zero_scores(shape[0], L, MC.rng_for(shape, mode, "szs")), None


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", MC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_forms_agree_and_cap_the_masked_count(shape, mode):
    """For every tie fixture and every k the GPU tests use: sort-threshold form == counting form == the oracle's statement of
    model_util.py:231-244; at most k entries are masked, and exactly k when there is no tie at rank k (sort[k-1] != sort[k])."""
    n = shape[0]
    L, count = MC.row_len(shape, mode), MC.summands(shape, mode)
    seen = set()
    for fx, score, T in _fixture_scores(shape, mode):
        seen.add(fx)
        assert score.dtype == np.float32 and score.shape == (n, L)
        if T is not None:          # the exact fp32 score is the mean up to its two roundings, and orders / ties exactly like the integer sums
            assert (np.abs(score.astype(np.float64) - T / count) <= 2.0 ** -23 * np.abs(T / count)).all()
            for r in range(n):
                assert np.array_equal(np.unique(T[r], return_inverse=True)[1], np.unique(score[r], return_inverse=True)[1])
        noise = MC.rng_for(shape, mode, fx, "noise").random((n, L), dtype=np.float32)
        srt = -np.sort(-score, axis=1)
        ks = MC.all_ks("random" if T is None else fx, score) + [ref_mask.clamp_k(k, L) for k in MC.device_ks_outside(L)]
        for k in ks:
            for soft in (None, noise):
                a, b = ref_mask.select(score, k, soft), ref_mask.select_by_count(score, k, soft)
                st = None if soft is None else torch.from_numpy(soft)
                c = ref_cpu.rank_select_mask(torch.from_numpy(score), k, st).numpy()
                assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32)), (fx, k)
                assert np.array_equal(a.view(np.int32), c.view(np.int32)), (fx, k)
            hit = (ref_mask.select(score, k) == 0).sum(axis=1)
            assert (hit <= k).all(), (fx, k)
            no_tie = (srt[:, k - 1] != srt[:, k]) if k > 0 else np.ones(n, dtype=bool)
            assert np.array_equal(hit == k, no_tie), (fx, k)
        if fx == "all_equal":
            assert all((ref_mask.select(score, k) == 1).all() for k in ks)
        if fx == "pairs":
            sp = MC.special_ks(fx, score)
            assert len(sp) == 2 and srt[0, sp[0]] == srt[0, sp[0] - 1] and srt[0, sp[1]] == srt[0, sp[1] + 1]
        if fx == "random" and L > 1:
            (k,) = MC.special_ks(fx, score)
            assert srt[0, k] != srt[0, k - 1] and (ref_mask.select(score[:1], k) == 0).sum() == k
    assert seen >= {fx for fx in MC.FIXTURES if L >= MC.MIN_LEN[fx]}


def test_apply_and_score_restatements():
    rng = np.random.default_rng(5)
    grad = rng.integers(-3, 4, (2, 6, 8)).astype(np.float32)
    for mode in (0, 1):
        s64 = ref_mask.score(grad, mode)
        assert s64.dtype == np.float64 and s64.shape == ((2, 8) if mode == 0 else (2, 6))
        assert np.array_equal(s64, torch.from_numpy(grad).double().mean(1 if mode == 0 else 2).numpy())
        inv = np.float32(1.0) / np.float32(6 if mode == 0 else 8)
        assert np.array_equal(ref_mask.score_exact_f32(grad, mode), grad.astype(np.float64).sum(1 if mode == 0 else 2).astype(np.float32) * inv)
        mask = rng.random(s64.shape).astype(np.float32)
        ref = torch.from_numpy(grad).permute(0, 2, 1) * (torch.from_numpy(mask)[:, :, None] if mode == 0 else torch.from_numpy(mask)[:, None, :])
        assert np.array_equal(ref_mask.apply(grad, mask, mode), ref.permute(0, 2, 1).numpy())


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9, 0.999])
def test_dropout_restatement_against_torch(p):
    g = torch.Generator().manual_seed(3)
    z = torch.randn(3, 5, 8, generator=g)
    z[0, 0, :4] = torch.tensor([0.0, -0.0, 1.0, -2.5])
    keep = (torch.rand(3, 8, generator=g) >= p).float()
    inv = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32))
    ref = z * (keep * inv)[:, None, :]
    out, full = ref_mask.dropout2d(z.numpy(), keep.numpy(), p)
    assert np.array_equal(out.view(np.int32), ref.numpy().view(np.int32))
    assert np.array_equal(full, (ref == z).float().numpy())
    zb = z.bfloat16()
    refb = (zb.float() * (keep * inv)[:, None, :]).bfloat16()
    outb, none = ref_mask.dropout2d(zb.float().numpy(), keep.numpy(), p, bf16_in=True, bf16_out=True)
    assert none is None and np.array_equal(outb.view(np.int16), refb.view(torch.int16).numpy())
    assert np.array_equal(ref_mask.from_bf16_bits(outb), refb.float().numpy())


# ================================================================================================ golden records
@pytest.fixture(scope="module")
def io_cases():
    return torch.load(os.path.join(GOLDEN, "io_cases.pt"), weights_only=False)


def test_ref_io_reproduces_the_recorded_results(io_cases):
    assert len(io_cases["rescale"]) and len(io_cases["crop_or_pad"]) and len(io_cases["noise_clamp"]) and len(io_cases["running_score"])
    for r in io_cases["rescale"]:
        x = r["x"].numpy()
        planes = x.shape[0] * x.shape[1]
        y = ref_io.rescale(x.reshape(planes, -1), r["new_min"], r["new_max"]).reshape(x.shape)
        assert np.array_equal(y.view(np.int32), r["y"].numpy().view(np.int32))
    for r in io_cases["crop_or_pad"]:
        assert np.array_equal(ref_io.crop_or_pad(r["image"].numpy(), *r["size"]).view(np.int32), r["image_out"].numpy().view(np.int32))
        assert np.array_equal(ref_io.crop_or_pad(r["label"].numpy(), *r["size"]), r["label_out"].numpy())
    for r in io_cases["noise_clamp"]:
        out = ref_io.noise_clamp(r["clean"].numpy(), r["noise"].numpy())
        assert np.array_equal(out.view(np.int32), r["out"].numpy().view(np.int32))
    for r in io_cases["running_score"]:
        n_class = r["confusion"].shape[0]
        hist = np.zeros((n_class, n_class), dtype=np.int64)
        for lt, lp in r["batches"]:
            hist = ref_io.confusion(lt.numpy(), lp.numpy(), n_class, hist)
        assert np.array_equal(hist, r["confusion"].numpy().astype(np.int64))


def test_ref_io_edges():
    lt = np.array([-1, 0, 1, 2, 2 ** 40 + 1, 1, 0], dtype=np.int64)
    lp = np.array([0, 1, 1, 0, 0, 255, 2], dtype=np.uint8)
    assert ref_io.confusion(lt, lp, 2).tolist() == [[0, 1], [0, 1]]
    assert ref_io.confusion(lt, lp, 1).tolist() == [[0]]
    x = np.full((1, 7), 3.5, dtype=np.float32)
    assert np.array_equal(ref_io.rescale(x, 0.25, 1.0), np.full((1, 7), 0.25, dtype=np.float32))      # constant plane: 0 / eps
    src = np.arange(1, 13, dtype=np.int64).reshape(1, 3, 4)
    assert ref_io.crop_or_pad(src, 4, 2).tolist() == [[[0, 0], [2, 3], [6, 7], [10, 11]]]               # floor(-1 / 2) = -1: pad on top
    assert ref_io.crop_or_pad(src, 2, 5).tolist() == [[[0, 1, 2, 3, 4], [0, 5, 6, 7, 8]]]
