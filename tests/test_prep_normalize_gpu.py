"""Percentiles and percentile normalisation on the device (ctl_order_stats + ctl_percentile_apply behind ops.percentile and
ops.percentile_normalize) against the host statements of prepare.py, which tests/test_prep_host_cpu.py pins to np.percentile of the
float64 values and to upstream's arithmetic.

Both sides do the same fp64 operations on exact order statistics and the same float32 operations with one rounding each, so every
comparison is bit for bit over every element.  The one thing left to the platform is the sign / payload of a NaN that 0 / 0 produces
(q = (50, 50) on a volume away from zero: hi == lo and the 1e-10 is absorbed): there both sides must hold a NaN."""
import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import ops, prepare

pytestmark = pytest.mark.gpu
F32 = np.float32
VOLUMES = [(3, 20, 24), (10, 64, 56), (1, 16, 16)]
QS = [(2, 98), (1, 95), (0, 100), (50, 50)]


def volume(shape, seed=0):
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    x = rng.gamma(2.0, 120.0, size=shape).astype(F32)
    x[rng.random(shape) < 0.3] = 0                                 # ties at the low percentiles
    x[0, 0, :4] = (-3.5, -0.0, 1e-40, 7e4)
    return x


def same_bits(got, want, what):
    """bit-equal over every element; where the host statement holds a NaN the device must hold one too"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("shape", VOLUMES, ids=str)
def test_percentile_is_bit_equal_to_the_host_statement(shape):
    x = volume(shape)
    for segments in (1, shape[0]):
        for q in ([0, 1, 2, 50, 98, 99, 100], [37.5], [2, 98], [25, 50, 75]):
            got = ops.percentile(dev(x), q, segments=segments)
            assert got.dtype == torch.float32 and tuple(got.shape) == (segments, len(q))
            same_bits(got.cpu().numpy(), prepare.percentile_host(x, q, segments=segments), (shape, segments, q))


@pytest.mark.parametrize("form", ["minmax", "medic"])
@pytest.mark.parametrize("shape", VOLUMES, ids=str)
def test_normalize_is_bit_equal_to_the_host_statement(shape, form):
    x = volume(shape, 1)
    xd = dev(x)
    for segments in (1, shape[0]):
        for q in QS:
            for new_min, new_max in ((0.0, 1.0), (-1.0, 2.5)) if form == "medic" else ((0.0, 1.0),):
                got, bounds = ops.percentile_normalize(xd, q, form=form, segments=segments, new_min=new_min, new_max=new_max, want_bounds=True)
                want, want_bounds = prepare.percentile_normalize_host(x, q, form=form, segments=segments, new_min=new_min, new_max=new_max,
                                                                      want_bounds=True)
                what = (shape, form, segments, q, new_min, new_max)
                assert tuple(got.shape) == shape and tuple(bounds.shape) == (segments, 2)
                same_bits(bounds.cpu().numpy(), want_bounds, what)
                same_bits(got.cpu().numpy(), want, what)
                if q != (50, 50):
                    assert np.isfinite(want).all(), what
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))           # the input is left alone


@pytest.mark.parametrize("form", ["minmax", "medic"])
def test_constant_volume_is_decided_by_the_eps_terms(form):
    """hi == lo: minmax divides 0 by 1e-10 (zero volume), medic multiplies by 1e8 and adds b = new_max - 1e8 * hi: finite, and the
    host statement's bits."""
    for value in (0.0, 2.0 ** -20):
        x = np.full((3, 20, 24), value, dtype=F32)
        for segments in (1, 3):
            got = ops.percentile_normalize(dev(x), (2, 98), form=form, segments=segments).cpu().numpy()
            want = prepare.percentile_normalize_host(x, (2, 98), form=form, segments=segments)
            assert np.isfinite(want).all() and np.isfinite(got).all()
            same_bits(got, want, (form, value, segments))


def test_out_argument_and_refusals():
    x = dev(volume((3, 20, 24), 2))
    out = torch.full_like(x, float("nan"))
    back = ops.percentile_normalize(x, (2, 98), out=out)
    assert back is out and torch.equal(out, ops.percentile_normalize(x, (2, 98)))
    with pytest.raises(ValueError):
        ops.percentile_normalize(x, (2, 98), out=x)
    with pytest.raises(ValueError):
        ops.percentile_normalize(x, (2, 98), out=out.double())
    with pytest.raises(ValueError):
        ops.percentile_normalize(x, (2, 50, 98))
    with pytest.raises(ValueError):
        ops.percentile(x, [101])
    with pytest.raises(ValueError):
        ops.percentile_normalize(x, (2, 98), segments=7)
