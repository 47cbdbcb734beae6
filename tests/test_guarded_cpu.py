"""oracle/guarded.py on CPU tensors: every check is shown to fail on a planted defect and to pass on a clean buffer, so that a green
guard-band test on the GPU (tests/test_*_guard_gpu.py) means something."""
import pytest
import torch

from oracle.guarded import GUARD_BYTE, GUARD_BYTES, Guarded, GuardedCall, GuardError, flat_with_gaps

DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32, torch.int64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("numel", [1, 7, 63, 1000])
def test_layout_alignment_exact_length_and_patterns(dtype, numel):
    g = Guarded(numel, dtype)
    assert g.ptr % 256 == 0
    assert g.flat().numel() == numel and g.flat().data_ptr() == g.ptr and g.nbytes == numel * g.itemsize
    assert g._front().numel() == GUARD_BYTES and g._back().numel() == GUARD_BYTES
    assert g._front().data_ptr() + GUARD_BYTES == g.ptr and g._back().data_ptr() == g.ptr + g.nbytes      # no rounding up, no slack
    assert bool((g._front() == GUARD_BYTE).all()) and bool((g._back() == GUARD_BYTE).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(g.flat()).all()), "float poison is a NaN"
        bits = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5, torch.float64: 0x7FF85A5A5A5A5A5A}[dtype]
        assert bool((g.bits() == bits).all())
    else:
        assert bool((g._payload_bytes() == 0x5A).all())
    z = Guarded(numel, dtype, poison=False)
    assert bool((z._payload_bytes() == 0).all())
    z.check_guards()


def test_views_share_the_payload():
    g = Guarded(2 * 3 * 4 * 5, torch.float32)
    v = g.view((2, 5, 3, 4), channels_last=True)                           # logical NCHW, memory NHWC
    assert v.shape == (2, 5, 3, 4) and v.is_contiguous(memory_format=torch.channels_last) and v.data_ptr() == g.ptr
    v.copy_(torch.arange(120.0).view(2, 5, 3, 4))
    assert float(g.flat()[1]) == float(v[0, 1, 0, 0]) == 12.0             # the channel is the fastest axis in memory
    p = g.view((6, 20))
    assert p.data_ptr() == g.ptr and p.is_contiguous()
    g.check_guards()
    g.check_written()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_one_byte_in_the_front_guard_is_reported_with_side_and_offset(dtype):
    g = Guarded(100, dtype)
    g.flat().zero_()
    g._buf[g._start - 3] = 0
    with pytest.raises(GuardError) as e:
        g.check_guards()
    assert e.value.violations == [dict(side="front", first=-3, last=-3, count=1)]
    assert "front guard" in str(e.value) and "-3" in str(e.value)
    g.check_written()                                                      # the payload itself is fine


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_one_byte_in_the_back_guard_is_reported_with_side_and_offset(dtype):
    g = Guarded(100, dtype)
    g.flat().zero_()
    g._buf[g._start + g.nbytes + 5] = 0
    with pytest.raises(GuardError) as e:
        g.check_guards()
    assert e.value.violations == [dict(side="back", first=g.nbytes + 5, last=g.nbytes + 5, count=1)]
    assert "back guard" in str(e.value)
    # the far ends of both guards are watched too, and both sides are reported together
    g.repoison()
    g._buf[g._start - GUARD_BYTES] = 1
    g._buf[g._start + g.nbytes + GUARD_BYTES - 1] = 1
    assert g.guard_violations() == [dict(side="front", first=-GUARD_BYTES, last=-GUARD_BYTES, count=1),
                                    dict(side="back", first=g.nbytes + GUARD_BYTES - 1, last=g.nbytes + GUARD_BYTES - 1, count=1)]


def test_a_row_written_past_the_end_is_reported_as_exactly_its_bytes():
    """what the GPU bite tests rely on: a payload declared one row of 16 floats short"""
    rows, c = 9, 16
    g = Guarded((rows - 1) * c, torch.float32)
    torch.as_strided(g.flat(), (rows, c), (c, 1)).fill_(1.0)      # the writer believes in `rows` rows (no byte of 1.0f is the guard's 0x5A)
    v = g.guard_violations()
    assert v == [dict(side="back", first=g.nbytes, last=g.nbytes + 4 * c - 1, count=4 * c)]
    g.check_written()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_unwritten_element_is_reported_with_its_index(dtype):
    g = Guarded(500, dtype)
    g.flat().copy_(torch.arange(500) % 50)
    g.check_written()
    g.poison_range(123, 124)
    with pytest.raises(GuardError) as e:
        g.check_written()
    assert e.value.violations == [dict(side="payload", count=1, indices=[123])] and "[123]" in str(e.value)
    g.check_guards()


def test_many_unwritten_elements_count_and_first_indices():
    g = Guarded(4096, torch.float32)
    g.flat()[:4000] = 1.0
    with pytest.raises(GuardError) as e:
        g.check_written()
    assert e.value.violations[0]["count"] == 96 and e.value.violations[0]["indices"] == list(range(4000, 4008))


def test_a_computed_nan_is_not_mistaken_for_poison():
    g = Guarded(64, torch.float32)
    x = torch.zeros(64)
    g.flat().copy_(x / x)                                                  # 0 / 0: the default quiet NaN, other payload bits
    assert bool(torch.isnan(g.flat()).all())
    g.check_written()
    h = Guarded(64, torch.bfloat16)
    h.flat().copy_((x / x).to(torch.bfloat16))
    h.check_written()
    g.flat()[7] = float("inf") - float("inf")
    g.check_written()


def test_zeroed_payload_refuses_the_written_check():
    g = Guarded(8, torch.float32, poison=False)
    with pytest.raises(RuntimeError):
        g.check_written()


def test_repoison_restores_payload_and_guards():
    g = Guarded(33, torch.float32)
    g.flat().fill_(2.0)
    g._buf[g._start - 1] = 0
    g._buf[g._start + g.nbytes] = 0
    snap = g.snapshot()
    g.repoison()
    g.check_guards()
    assert g.unwritten().numel() == 33 and bool((snap.view(torch.float32) == 2.0).all()), "the snapshot is a copy"


def test_flat_with_gaps_layout_and_gap_write():
    f = flat_with_gaps([100, 64, 1, 200])
    assert f.offsets == [0, 128, 192, 256] and f.total == 512
    assert f.ptr % 256 == 0 and f.range_ptr(2) == f.ptr + 4 * 192
    for i in range(4):
        f.range(i).fill_(float(i + 1))
    f.check_guards()
    for i in range(4):
        f.check_written(i)
    assert f.range(3, (10, 20)).shape == (10, 20)
    f.flat()[100] = 0.0                                                    # first float of the gap behind range 0
    with pytest.raises(GuardError) as e:
        f.check_guards()
    assert e.value.violations == [dict(side="gap", after_range=0, first=100, last=100, count=1)]
    f.flat()[100] = float("nan")                                           # a NaN with other bits is still a write
    assert f.gap_violations()[0]["count"] == 1
    f.repoison()
    f.range(1).fill_(3.0)
    f.flat()[193:196] = 5.0                                                # behind the one-float range 2
    assert f.gap_violations() == [dict(side="gap", after_range=2, first=193, last=195, count=3)]
    with pytest.raises(GuardError):
        f.check_written(0)                                                 # repoisoned and not written again
    f.check_written(1)


def test_flat_with_gaps_outer_guard_and_unwritten_range_element():
    f = flat_with_gaps([64, 64])                                           # no gaps at all: the outer guards still stand
    f.range(0).fill_(1.0)
    f.range(1).fill_(1.0)
    f.check_guards()
    f.buf._buf[f.buf._start + f.buf.nbytes] = 0
    with pytest.raises(GuardError) as e:
        f.check_guards()
    assert e.value.violations[0]["side"] == "back"
    f.repoison()
    f.range(0).fill_(1.0)
    f.range(1)[:63] = 1.0
    with pytest.raises(GuardError) as e:
        f.check_written(1)
    assert e.value.violations == [dict(side="payload", range=1, count=1, indices=[63])]


def test_a_clean_run_passes_every_check():
    g = Guarded(3 * 16 * 9 * 7, torch.float32)
    y = g.view((3, 16, 9, 7), channels_last=True)
    y.copy_(torch.randn(3, 16, 9, 7))
    first = g.snapshot()
    g.check_guards()
    g.check_written()
    g.repoison()
    y.copy_(y.new_zeros(()).expand_as(y) + first.view(torch.float32).view(3, 9, 7, 16).permute(0, 3, 1, 2))
    assert torch.equal(g.snapshot(), first)
    g.check_guards()
    g.check_written()


def test_guarded_call_runs_the_steps_and_sees_each_defect():
    """GuardedCall, the harness of the GPU files: a clean producer passes run and rerun; an overrun, a skipped element, a changed gap of a
    flat buffer and a run-to-run difference are each reported"""
    def case(defect=None):
        gc = GuardedCall("cpu")
        y = gc.out("y", 40)
        acc = gc.out("acc", 8, init=lambda b: b.flat().fill_(1.0))
        loose = gc.out("loose", 16, written=False)                     # guards only: padding nobody reads may stay unwritten
        flat = gc.flat("grad", [10, 70, 3], written=[1], init=lambda f: (f.range(0).fill_(7.0), f.range(2).fill_(9.0)))
        calls = []

        def launch():
            calls.append(1)
            y.flat().copy_(torch.arange(40.0))
            acc.flat().add_(2.0)
            loose.flat()[:4] = 0.0
            flat.range(1).fill_(3.0)
            if defect == "overrun":
                torch.as_strided(y.flat(), (41,), (1,))[40] = 5.0
            if defect == "skipped":
                y.poison_range(17, 18)
            if defect == "gap":
                flat.flat()[10] = 0.0
            if defect == "second run differs" and len(calls) == 2:
                y.flat()[3] = -1.0
        return gc, launch, acc, flat

    gc, launch, acc, flat = case()
    gc.run(launch).rerun(launch)
    assert bool((acc.flat() == 3.0).all()), "the accumulator's previous contents are restored before the second run"
    assert bool((flat.range(0) == 7.0).all()) and bool((flat.range(2) == 9.0).all())
    for defect, side in (("overrun", "back"), ("skipped", "payload"), ("gap", "gap")):
        gc, launch, _, _ = case(defect)
        with pytest.raises(GuardError) as e:
            gc.run(launch)
        assert e.value.violations[0]["side"] == side, (defect, e.value.violations)
    gc, launch, _, _ = case("second run differs")
    gc.run(launch)
    with pytest.raises(GuardError) as e:
        gc.rerun(launch)
    assert e.value.violations == [dict(side="rerun", count=1)] and "y" in str(e.value)
