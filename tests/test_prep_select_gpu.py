"""Exact order statistics on the device (ctl_order_stats behind ops.order_statistics): the radix select against np.sort.

Every comparison is numerical equality with the sorted segment at the asked ranks (np.array_equal: bit-equal except for the sign of a
zero, which np.sort does not order; the order of -0.0 and +0.0 has a test of its own).  The output table and the workspace are
guard-banded, poisoned buffers (oracle/guarded.py) of exactly the sizes the C-ABI states, and every call is repeated for identical bytes."""
import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops, prepare
from oracle.guarded import GuardedCall

pytestmark = pytest.mark.gpu
lib, check = _ffi.lib, _ffi.check
F32 = np.float32
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 35840, 2 ** 20 + 3]
CONTENTS = ["normal", "negative", "zeros_gamma", "constant", "consecutive", "top_byte", "specials"]


def content(name, n, rng):
    if name == "normal":                                           # both signs
        return (rng.standard_normal(n) * 100).astype(F32)
    if name == "negative":
        return (-np.abs(rng.standard_normal(n)) * 100 - 1).astype(F32)
    if name == "zeros_gamma":                                      # MRI-like: 70 % exact zeros plus a gamma tail
        x = rng.gamma(2.0, 100.0, size=n).astype(F32)
        x[rng.random(n) < 0.7] = 0
        return x
    if name == "constant":
        return np.full(n, 3.25, dtype=F32)
    if name == "consecutive":                                      # consecutive floats: only the last digit passes separate them
        return (np.uint32(0x42000000) + rng.permutation(n).astype(np.uint32)).view(F32)
    if name == "top_byte":                                         # differ only in the top byte (sign and 7 exponent bits); finite: bit 23 is 0
        return ((rng.integers(0, 256, size=n).astype(np.uint32) << 24) | np.uint32(0x00345678)).view(F32)
    if name == "specials":
        fi = np.finfo(F32)
        pool = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45, fi.tiny, -fi.tiny, fi.max, -fi.max, 1.0, -1.0], dtype=F32)
        return pool[rng.integers(0, pool.size, size=n)]
    raise KeyError(name)


def rank_sets(n, x=None):
    k0, k0u, _ = ops.percentile_index(n, 2)
    k1, k1u, _ = ops.percentile_index(n, 98)
    sets = [[0], [n - 1], [0, n - 1], [k0, k0u, k1, k1u],
            [n - 1, 0, n // 2, n // 2, n // 3, n - 1, (2 * n) // 3, min(1, n - 1)]]          # 8 ranks, duplicates, unsorted
    if x is not None:                                              # the run of zeros: its first and last position, inside it, and just after
        s = np.sort(x)
        z = np.nonzero(s == 0)[0]
        if z.size:
            sets.append(sorted({int(z[0]), int(z[z.size // 2]), int(z[-1]), min(int(z[-1]) + 1, n - 1)}, reverse=True))
    return sets


def select(x, ranks):
    """ctl_order_stats on x [segments, n] through guarded buffers of the exact sizes, run twice -> table [segments, len(ranks)]"""
    segments, n = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rk = np.array(ranks, dtype=np.int64)
    nbytes = lib.ctl_order_stats_ws_bytes(segments, rk.size)
    assert nbytes == segments * 256 * (128 + 3 * rk.size) * 4
    gc = GuardedCall("cuda")
    out = gc.out("table", segments * rk.size)
    ws = gc.out("workspace", nbytes, dtype=torch.uint8, written=False)

    def launch():
        check(lib.ctl_order_stats(xd.data_ptr(), segments, n, rk.ctypes.data, rk.size, out.ptr, ws.ptr, nbytes,
                                  torch.cuda.current_stream().cuda_stream), "ctl_order_stats")
    gc.run(launch)
    got = out.view((segments, rk.size)).cpu().numpy().copy()
    gc.rerun(launch)                                               # guards, every table entry written, identical bytes (workspace included)
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))          # the input is left alone
    return got


@pytest.mark.parametrize("n", SIZES)
def test_single_segment_matches_sort(n):
    rng = np.random.default_rng(n)
    for name in CONTENTS:
        x = content(name, n, rng)
        s = np.sort(x)
        for ranks in rank_sets(n, x if name == "zeros_gamma" else None):
            got = select(x[None], ranks)
            assert got.shape == (1, len(ranks)) and np.array_equal(got[0], s[ranks]), (name, n, ranks, got[0], s[ranks])


@pytest.mark.parametrize("segments,n", [(5, 1000), (7, 255), (10, 3584)])
def test_segments_do_not_leak(segments, n):
    """a different distribution (and scale) in every segment: a count that leaked between segments would move a rank"""
    rng = np.random.default_rng(segments * n)
    x = np.stack([content(CONTENTS[i % len(CONTENTS)], n, rng) * F32(1 if CONTENTS[i % len(CONTENTS)] in ("top_byte", "specials") else 1 + i)
                  for i in range(segments)])
    s = np.sort(x, axis=1)
    for ranks in rank_sets(n):
        assert np.array_equal(select(x, ranks), s[:, ranks]), ranks
    t = ops.order_statistics(torch.from_numpy(x).cuda().reshape(segments, 1, n), [0, n - 1], segments=segments)
    assert t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), s[:, [0, n - 1]])


def test_negative_zero_sorts_before_positive_zero():
    x = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -0.0], dtype=F32)
    got = select(x[None], [0, 1, 2, 3, 4, 5])[0]
    assert np.array_equal(got.view(np.uint32), np.array([-0.0, -0.0, -0.0, 0.0, 0.0, 1.0], dtype=F32).view(np.uint32))


def test_python_layer_arguments():
    x = torch.zeros(10, device="cuda")
    for bad in ([], list(range(9)), [10], [-1]):
        with pytest.raises(_ffi.CtlError):
            ops.order_statistics(x, bad)
    with pytest.raises(ValueError):
        ops.order_statistics(x, [0], segments=3)
    with pytest.raises(TypeError):
        ops.order_statistics(x.double(), [0])
    strided = torch.arange(20, device="cuda", dtype=torch.float32)[::2]          # copied, not misread
    assert ops.order_statistics(strided, [9]).item() == 18


SHAPE = (10, 64, 56)                                               # 35840 elements: several blocks per segment as a whole, one per slice


def _inputs():
    rng = np.random.default_rng(2)
    n = int(np.prod(SHAPE))
    inputs = {k: content(k, n, rng).reshape(SHAPE) for k in ("normal", "zeros_gamma")}
    inputs["constant"] = np.zeros(SHAPE, dtype=F32)              # hi == lo == 0: the eps of the minmax form decides, 0 / 1e-10
    return inputs


@pytest.mark.parametrize("segments", [1, SHAPE[0]])
def test_launch_sequence_does_not_depend_on_the_content(segments):
    """Launch census of eager calls (5 for the select, 6 for select + apply, the same for random, constant and zero-heavy content), and
    ONE capture of both into a graph (a single chain), replayed after the static input is overwritten: every replay equals the host
    statement of the new content."""
    inputs = _inputs()
    static = torch.from_numpy(inputs["normal"]).cuda()
    seg_elems = static.numel() // segments
    ranks = [0, seg_elems // 2, seg_elems - 1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up outside the capture
        ops.order_statistics(static, ranks, segments=segments)
        ops.percentile_normalize(static, (2, 98), segments=segments, want_bounds=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        table = ops.order_statistics(static, ranks, segments=segments)
        norm, bounds = ops.percentile_normalize(static, (2, 98), segments=segments, want_bounds=True)
    census = set()
    for name in ("constant", "zeros_gamma", "normal"):
        static.copy_(torch.from_numpy(inputs[name]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        s = np.sort(inputs[name].reshape(segments, -1), axis=1)
        assert np.array_equal(table.cpu().numpy(), s[:, ranks]), name
        want, want_bounds = prepare.percentile_normalize_host(inputs[name], (2, 98), segments=segments, want_bounds=True)
        assert np.array_equal(bounds.cpu().numpy().view(np.uint32), want_bounds.view(np.uint32)), name
        assert np.array_equal(norm.cpu().numpy().view(np.uint32), want.view(np.uint32)), name
        before = lib.ctl_launch_count()
        ops.order_statistics(static, ranks, segments=segments)
        mid = lib.ctl_launch_count()
        ops.percentile_normalize(static, (2, 98), segments=segments)
        census.add((int(mid - before), int(lib.ctl_launch_count() - mid)))
    assert census == {(5, 6)}, census
