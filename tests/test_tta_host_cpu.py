"""The numpy statements of test-time augmentation (tta.views_host / tta.merge_host), which the kernels of csrc/ctl_tta.hip are tested
against: each view against the literal np.flip / np.transpose chain, the merge as the inverse of the views, the group structure of the
eight codes, the two means against independent statements, and the refusals of parse_views."""
import numpy as np
import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import tta, uncertainty as U

SETS = [(v,) for v in range(8)] + ["flips", "d4", (3, 5, 6)]

# code -> the literal chain on a plane [H, W] (bit 0 transpose, then bit 1 flip H, then bit 2 flip W)
LITERAL = {
    0: lambda p: p,
    1: lambda p: np.transpose(p),
    2: lambda p: np.flip(p, 0),
    3: lambda p: np.flip(np.transpose(p), 0),
    4: lambda p: np.flip(p, 1),
    5: lambda p: np.flip(np.transpose(p), 1),
    6: lambda p: np.flip(np.flip(p, 0), 1),
    7: lambda p: np.flip(np.flip(np.transpose(p), 0), 1),
}


def planes(n, c, h, w):
    """asymmetric content: every element distinct"""
    return np.arange(n * c * h * w, dtype=np.float32).reshape(n, c, h, w) * 0.5 - 7.0


def transposing(views):
    return any(v & 1 for v in tta.parse_views(views))


@pytest.mark.parametrize("hw", [(5, 7), (5, 5)])
def test_each_view_is_the_literal_flip_transpose_chain(hw):
    x = planes(2, 3, *hw)
    for v in range(8):
        if v & 1 and hw[0] != hw[1]:
            with pytest.raises(ValueError, match=f"view code {v}"):
                tta.views_host(x, (v,))
            continue
        got = tta.views_host(x, (v,))
        assert got.shape == x.shape and got.dtype == x.dtype
        for b in range(2):
            for k in range(3):
                assert np.array_equal(got[b, k], LITERAL[v](x[b, k])), (v, hw)
    # the formula of the header: view[y, x] = A[bit1 ? Ho-1-y : y, bit2 ? Wo-1-x : x]
    h, w = hw
    for v in (range(8) if h == w else (0, 2, 4, 6)):
        a = np.swapaxes(x, -1, -2) if v & 1 else x
        yy, xx = np.mgrid[0:h, 0:w]
        want = a[:, :, np.where(v & 2, h - 1 - yy, yy), np.where(v & 4, w - 1 - xx, xx)]
        assert np.array_equal(tta.views_host(x, (v,)), want), v


@pytest.mark.parametrize("views", SETS, ids=str)
@pytest.mark.parametrize("hw", [(5, 7), (5, 5)])
def test_the_merge_undoes_the_views(views, hw):
    if transposing(views) and hw[0] != hw[1]:
        with pytest.raises(ValueError, match="transposes"):
            tta.merge_host(planes(3 * len(tta.parse_views(views)), 2, *hw), views, hw, mode=None)
        return
    codes = tta.parse_views(views)
    x = planes(3, 2, *hw)
    stack = tta.views_host(x, views)
    assert stack.shape == (len(codes) * 3, 2) + hw
    for t, v in enumerate(codes):                                             # member-major
        assert np.array_equal(stack[t * 3:(t + 1) * 3], tta.views_host(x, (v,)))
    back = tta.merge_host(stack, views, hw, mode=None)
    assert back.merged is None and back.pred is None and back.aligned.dtype == x.dtype
    assert np.array_equal(back.aligned, np.concatenate([x] * len(codes), axis=0))
    # native pixel (i, j) is found in view v at (y, x) of the header's inverse formula
    h, w = hw
    for t, v in enumerate(codes):
        for i, j in ((0, 0), (1, 3), (h - 1, w - 2), (h - 1, w - 1)):
            a, b = (j, i) if v & 1 else (i, j)
            y, xx = (h - 1 - a if v & 2 else a), (w - 1 - b if v & 4 else b)      # (h == w whenever the code transposes)
            assert stack[t * 3 + 1, 1, y, xx] == x[1, 1, i, j], (v, i, j)


def predicted_inverse(v):
    """Transposing exchanges the two flips: native (i, j) sits in view v at (y, x) = (F1(j), F2(i)), so the view that undoes v is
    "transpose, flip H by bit 2, flip W by bit 1"; without the transpose a code undoes itself."""
    return (v & 1) | ((v & 4) >> 1) | ((v & 2) << 1) if v & 1 else v


def test_the_codes_are_a_group_and_the_inverse_is_the_predicted_one():
    probe = np.arange(16.0).reshape(1, 1, 4, 4)
    images = [tta.views_host(probe, (v,)) for v in range(8)]
    assert len({im.tobytes() for im in images}) == 8                          # eight different elements

    def compose(v, u):                                                        # the code of "view u, then view v"
        got = tta.views_host(images[u], (v,))
        return next(k for k in range(8) if np.array_equal(images[k], got))    # (StopIteration: not closed)

    table = [[compose(v, u) for u in range(8)] for v in range(8)]
    for v in range(8):
        assert sorted(table[v]) == list(range(8)) and sorted(row[v] for row in table) == list(range(8))      # a latin square: closed
        for u in range(8):
            assert np.array_equal(tta.views_host(tta.views_host(probe, (u,)), (v,)), images[table[v][u]])
        inv = predicted_inverse(v)
        assert table[inv][v] == 0 == table[v][inv]
        assert np.array_equal(tta.views_host(images[v], (inv,)), probe)
    assert [predicted_inverse(v) for v in range(8)] == [0, 1, 2, 5, 4, 3, 6, 7]       # "transpose, flip H" is undone by "transpose, flip W"
    assert table[3][3] != 0 and table[5][5] != 0


@pytest.mark.parametrize("views", ["flips", "d4", (3, 5, 6), (6,)], ids=str)
def test_prob_mode_is_the_mean_prob_of_the_uncertainty_statement(views):
    T = len(tta.parse_views(views))
    rng = np.random.default_rng(11 + T)
    logits = (rng.standard_normal((T * 3, 5, 6, 6)) * 3.0).astype(np.float32)
    logits[0, :, 0, 0] = (80.0, -80.0, 0.0, 0.0, 0.0)
    got = tta.merge_host(logits, views, (6, 6), mode="prob")
    ref = U.predictive_stats_host(got.aligned, members=T)
    assert got.merged.dtype == np.float64 and got.merged.shape == (3, 5, 6, 6)
    assert np.abs(got.merged - ref.mean_prob).max() <= 1e-15
    assert np.array_equal(got.pred, ref.pred) and got.pred.dtype == np.uint8
    assert np.abs(got.merged.sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("T", [1, 2, 4, 8])
def test_logit_mode_with_a_power_of_two_is_the_rounded_fp64_mean(T):
    """T a power of two: the division is exact, so the fp32 result is the fp32 sum.  On inputs that are multiples of 2^-10 below 64 every
    partial sum is exact in fp32 as well, and the literal fp32 sequence must equal the mean computed in fp64 and rounded to fp32."""
    views = tuple(range(8))[:T] if T > 1 else (6,)
    rng = np.random.default_rng(T)
    logits = (rng.integers(-(1 << 15), 1 << 15, size=(T * 2, 4, 5, 5)) / 1024.0).astype(np.float32)
    got = tta.merge_host(logits, views, (5, 5), mode="logit")
    assert got.merged.dtype == np.float32
    want = got.aligned.astype(np.float64).reshape(T, 2, 4, 5, 5).mean(axis=0).astype(np.float32)
    assert np.array_equal(got.merged.view(np.int32), want.view(np.int32))
    assert np.array_equal(got.pred, want.argmax(axis=1))
    # and on arbitrary fp32 values: within one rounding per add of the fp64 mean
    x = (rng.standard_normal((T * 2, 4, 5, 5)) * 3.0).astype(np.float32)
    got = tta.merge_host(x, views, (5, 5), mode="logit")
    exact = got.aligned.astype(np.float64).reshape(T, 2, 4, 5, 5).mean(axis=0)
    assert np.abs(got.merged - exact).max() <= T * 2.0 ** -24 * np.abs(got.aligned).max()
    if T <= 2:                                                                # one add: correctly rounded, so equal on any input
        assert np.array_equal(got.merged.view(np.int32), exact.astype(np.float32).view(np.int32))


def test_logit_mode_adds_in_member_order():
    x = np.zeros((3, 1, 1, 1), dtype=np.float32)
    x[:, 0, 0, 0] = (2.0 ** 24, 1.0, -2.0 ** 24)                               # (a + b) + c = 0, a + (b + c) = 1 in fp32
    assert tta.merge_host(x, (0, 2, 4), (1, 1), mode="logit").merged[0, 0, 0, 0] == 0.0
    assert tta.merge_host(x[[1, 2, 0]], (0, 2, 4), (1, 1), mode="logit").merged[0, 0, 0, 0] == np.float32(1.0) / np.float32(3.0)


def test_parse_views_refusals():
    assert tta.parse_views("flips") == (0, 2, 4, 6) == tta.VIEW_SETS["flips"]
    assert tta.parse_views("d4") == tuple(range(8))
    assert tta.parse_views([3, 5, 6]) == (3, 5, 6) and tta.parse_views((np.int64(7),)) == (7,)
    assert tta.parse_views((5,)) == (5,)                                      # the identity need not be a member
    for bad, word in (("rot90", "unknown view set"), ((), "0 views"), (tuple(range(8)) + (0,), "9 views"), ((0, 8), "view code 8"),
                      ((-1,), "view code -1"), ((0, 2, 2), "duplicate view code 2"), ((1.0,), "view code 1.0"), ((True,), "view code True"),
                      (3, "a set name or a tuple"), (None, "a set name or a tuple")):
        with pytest.raises(ValueError, match=word):
            tta.parse_views(bad)
    assert tta.parse_views("d4", (5, 5)) == tuple(range(8)) and tta.parse_views("flips", (5, 7)) == (0, 2, 4, 6)
    with pytest.raises(ValueError, match="view code 5 transposes, the plane 5 x 7"):
        tta.parse_views((0, 2, 5), (5, 7))
    with pytest.raises(ValueError, match="mode"):
        tta.merge_host(np.zeros((2, 1, 2, 2), np.float32), (0, 2), (2, 2), mode="mean")
    with pytest.raises(ValueError, match="expected"):
        tta.merge_host(np.zeros((3, 1, 2, 2), np.float32), (0, 2), (2, 2))
    with pytest.raises(ValueError, match="expected"):
        tta.merge_host(np.zeros((2, 1, 2, 3), np.float32), (0, 2), (2, 2))
