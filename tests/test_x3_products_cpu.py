"""The conditions tests/test_x3_products_gpu.py rests on, checked on the host for every case it runs and with the very operands it uses
(oracle/x3_products.py): the hi*hi products cancel exactly, borders included; the fp64 emulation of the six products the kernels keep is
within 4e-6 of the exact result; and every way of getting ONE of the six matrix instructions wrong -- a low-order product missing, a cross
term formed twice in place of its mirror image -- moves the result by at least 3e-4 of max|ref|.  These two figures are conditions on the
INPUTS (the emulation gives 1.0e-6 ... 3.5e-6 and >= 4.7e-4), not tolerances on device code: a case that misses them needs other
inputs."""
import pytest
import torch

from oracle import x3_products as X

E6_MAX, FIVE_MIN = 4e-6, 3e-4


def _conditions(e):
    assert e.big_zero == 0.0, f"op(big_x, big_w) is not identically zero (max {e.big_zero})"
    assert e.check_err <= 1e-12, f"the emulated operation is not the operation: {e.check_err:.2e} off torch's own formulation"
    assert e.e6 < E6_MAX, f"six products: {e.e6:.2e} of max|ref|"
    for name, err in e.five.items():
        assert err >= FIVE_MIN, f"'{name}' moves the result by only {err:.2e} of max|ref|: the inputs do not discriminate"
    # the two dominant cross terms are most of the result, the three low-order products about 1e-3 of it
    assert e.five["drop hm"] > 0.05 and e.five["drop mh"] > 0.05
    print(f"{e.case.name}: e6 {e.e6:.2e}  five-product variants {e.five_min:.2e} ... {max(e.five.values()):.2e}  residual hi*hi {e.hh_max:.1e}")


def test_split3_is_exact_and_every_plane_is_live():
    g = torch.Generator().manual_seed(1)
    x = X.with_tail(X._bigs((4096,), g), g)
    hi, mid, lo = X.split3(x)
    assert set(hi.abs().tolist()) == {1.0, 2.0, 3.0}
    assert float(mid.abs().max()) <= 2.0 ** -8 and float((mid != 0).double().mean()) > 0.99
    assert float(lo.abs().max()) <= 2.0 ** -16 and float((lo != 0).double().mean()) > 0.9
    s = X.with_tail(X._bigs((4096,), g, (1,)), g, 2.0 ** -21, 8192, True)          # the operands of the summing packs
    hi, mid, lo = X.split3(s)
    assert set(hi.abs().tolist()) == {1.0} and float((lo != 0).double().mean()) > 0.8          # (13 tail bits: 8 in mid, 5 in lo)
    four = s.view(-1, 4).double().sum(1)
    assert torch.equal(four.float().double(), four), "a sum of four such weights must be an fp32 number"


def test_a_tail_towards_zero_from_one_is_the_case_the_builder_has_to_handle():
    """bf16 is twice as fine below a power of two: 1 - 2^-8 is a bf16 number, so hi != big for an unhalved tail"""
    x = torch.tensor([1.0 - 2.0 ** -8 + 2.0 ** -20, -1.0 + 2.0 ** -8 - 2.0 ** -20])
    assert X.split3(x)[0].abs().tolist() == [1.0 - 2.0 ** -8] * 2


@pytest.mark.parametrize("c", X.FWD_CASES, ids=[c.name for c in X.FWD_CASES])
def test_forward_case_inputs_discriminate(c):
    e = X.forward_case(c)
    assert tuple(e.x.shape) == (c.n, c.cin, c.h, c.w) and e.x.dtype == torch.float32 and e.w.dtype == torch.float32
    _conditions(e)


WG = X.WGRAD_CASES + list(X.GROUP_PAIR)


@pytest.mark.parametrize("c", WG, ids=[c.name for c in WG])
def test_weight_gradient_case_inputs_discriminate(c):
    e = X.wgrad_case(c)
    assert tuple(e.x.shape) == (c.n, c.cin, c.h, c.w) and tuple(e.ref.shape) == (c.cout, c.cin, c.ks, c.ks)
    _conditions(e)

