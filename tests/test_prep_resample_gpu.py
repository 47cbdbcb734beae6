"""In-plane resampling on the device (ctl_resample_inplane behind ops.resample_inplane) against prepare.resample_inplane_host, which
tests/test_prep_host_cpu.py pins to scipy's map_coordinates.

Labels: exactly equal, no pixel excluded (the coordinate is the same single fp64 multiply on both sides).  Image: within one float32
ulp of the result's magnitude at every pixel -- the results are positive sums of positive terms, so that is no wider than one ulp of
the larger neighbour; the fp64 summation order is the only freedom, and the measured distance is printed."""
import numpy as np
import pytest
import torch

from cooperative_training_and_latent_space_data_augmentation_amd import ops, prepare

pytestmark = pytest.mark.gpu
F32 = np.float32

# (shape, spacing, new_spacing): ratios 0.8 and 1.25; anisotropic; the last output column reads c = 23.4 in the band [23, 23.5);
# the last output column reads c = 23.56 >= 23.5: zero; upstream's own preparation of an ACDC volume
CASES = [((2, 20, 24), (1.0, 1.0, 10.0), (0.8, 0.8, -1)), ((2, 20, 24), (1.0, 1.0, 10.0), (1.25, 1.25, -1)),
         ((3, 33, 17), (1.0, 1.0, 8.0), (0.7, 1.2, -1)), ((2, 20, 24), (1.0, 1.0, 10.0), (0.78, 1.0, -1)),
         ((2, 20, 24), (1.0, 1.0, 10.0), (0.76, 0.93, -1)), ((6, 40, 36), (1.5625, 1.5625, 10.0), (1.36719, 1.36719, -1)),
         ((1, 25, 27), (2.0, 3.0, 5.0), (4.0, 6.0, -1))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64], ids=["uint8", "int64"])
@pytest.mark.parametrize("shape,spacing,new_spacing", CASES, ids=str)
def test_resample_matches_the_host_statement(shape, spacing, new_spacing, label_dtype):
    rng = np.random.default_rng(int(np.prod(shape)))
    image = (rng.gamma(2.0, 100.0, size=shape) + 1).astype(F32)          # positive: an outside zero cannot pass for a sample
    label = rng.integers(1, 4, size=shape).astype(label_dtype)
    want, want_label, want_sp = prepare.resample_inplane_host(image, spacing, new_spacing, label=label)
    got, got_label, sp = ops.resample_inplane(dev(image), spacing, new_spacing, label=dev(label))
    assert sp == want_sp and tuple(got.shape) == want.shape and got.dtype == torch.float32 and got_label.dtype == dev(label).dtype
    assert np.array_equal(got_label.cpu().numpy(), want_label)
    g = got.cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(g), np.abs(want)))
    print("  %s -> %s: max |diff| %.2f ulp, %d pixels outside" % (shape, want.shape, float((np.abs(g - want) / ulp).max()), int((want == 0).sum())))
    assert (np.abs(g - want) <= ulp).all()
    assert np.array_equal(g == 0, want == 0)
    only, none, _ = ops.resample_inplane(dev(image), spacing, new_spacing)
    assert none is None and torch.equal(only, got)


def test_band_and_beyond_are_exercised():
    image = np.arange(1, 1 + 24, dtype=F32)[None, None, :].repeat(4, axis=1)
    band, _, _ = ops.resample_inplane(dev(image), (1, 1, 1), (0.78, 1.0, -1))
    assert tuple(band.shape) == (1, 4, 31) and bool((band[0, :, 30] == 24).all())
    beyond, _, _ = ops.resample_inplane(dev(image), (1, 1, 1), (0.76, 1.0, -1))
    assert tuple(beyond.shape) == (1, 4, 32) and bool((beyond[0, :, 31] == 0).all()) and bool((beyond[0, :, 30] > 23).all())


def test_identity_slice_axis_and_arguments():
    image, label = dev(np.ones((3, 33, 17), dtype=F32)), dev(np.ones((3, 33, 17), dtype=np.int64))
    out, lab, sp = ops.resample_inplane(image, (1.25, 1.25, 10), (1.25, 1.25004, -1), label=label)
    assert out is image and lab is label and sp == (1.25, 1.25, 10.0)
    assert ops.resample_inplane(image, (1.0, 1.0, 8.0), (0.7, 1.3, -1))[0] is image          # upstream's rule is about the SUM of the scalings
    with pytest.raises(NotImplementedError):
        ops.resample_inplane(image, (1.25, 1.25, 10), (1.0, 1.0, 10.0), label=label)
    with pytest.raises(ValueError):
        ops.resample_inplane(image, (1.25, 1.25, 10), (1.0, 1.0, -1), label=label.int())
    with pytest.raises(ValueError):
        ops.resample_inplane(image.double(), (1.25, 1.25, 10), (1.0, 1.0, -1))
    with pytest.raises(ValueError):
        ops.resample_inplane(image[0], (1.25, 1.25, 10), (1.0, 1.0, -1))
