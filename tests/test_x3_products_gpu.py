"""CTL_DT_X3, product by product: does every kernel form that spells out the six matrix instructions
hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi (csrc/ctl_conv_x3_stage.h) really form these six?

tests/test_x3_gpu.py holds the X3 kernels to max(2 e0, 2e-6) of max|ref| on Gaussian data, where a missing low-order product moves the
result by 2.5e-6: it cannot tell six products from five.  Here the operands are built so that the hi*hi products cancel exactly
(oracle/x3_products.py); what is left are the cross terms, and each of mid*mid, hi*lo, lo*hi carries about 1e-3 of the result.  Per case:

    e3, e0   max error of the X3 kernel / the fp32-MFMA kernel on the same descriptor against the fp64 reference, relative to max|ref|
    e6       the same error of the host emulation of the six products (fp64 on exact bf16 planes, one rounding to fp32)
    five     the smallest such error over the seven ways of getting ONE matrix instruction wrong (a low-order product missing, a cross
             term formed twice in place of its mirror image)
    T = max(2 e0, 4 e6): the rule of test_x3_gpu.py::errs, with a floor that comes from the emulation and not from the kernel under test

    1. five >= 5 T, or the inputs do not discriminate (a condition on the inputs, checked on every run)
    2. e3 <= T

and the form that ran is the form the case is about (the profiling id of the launch: kernel family, kernel size, stride, input mode, pixel
tile, cout tiles per block, epilogue class, two-tensor prologue).  Prologues, virtual gradients and epilogues run with identity side inputs:
their code path is taken, the bf16 structure of the operand is not disturbed.  tests/test_x3_products_cpu.py checks the conditions on the
inputs without a GPU.

Measured on an MI355X (first green run; e3 / e0 / e6 / five, ratio = five / T):
    case                      e3        e0        e6        five     ratio
    s1_4x16_nt1               4.09e-06  2.74e-05  1.53e-06  6.75e-04   12.3
    s1_4x16_nt1_ragged        4.12e-06  2.25e-05  1.29e-06  7.11e-04   15.8
    s1_4x16_nt1_cout4         4.61e-06  2.79e-05  1.43e-06  7.23e-04   13.0
    s1_4x16_nt2               5.35e-06  2.90e-05  1.73e-06  7.23e-04   12.5
    s1_8x16_nt1               3.61e-06  2.74e-05  1.39e-06  6.39e-04   11.7
    s1_8x16_nt2_ragged        4.05e-06  3.17e-05  1.53e-06  7.36e-04   11.6
    s1_8x32_nt1               3.88e-06  2.84e-05  1.60e-06  7.18e-04   12.6
    s1_8x32_nt2               3.53e-06  2.97e-05  1.46e-06  6.85e-04   11.5
    s1_bnbwd_x2               3.93e-06  2.76e-05  1.40e-06  7.09e-04   12.9
    pc_4x16                   6.59e-06  2.42e-05  1.43e-06  6.41e-04   13.2
    pc_8x16                   6.85e-06  2.57e-05  1.37e-06  7.25e-04   14.1
    pc_8x32                   5.08e-06  2.60e-05  1.52e-06  7.09e-04   13.6
    pc_bnbwd                  6.75e-06  2.68e-05  1.48e-06  6.97e-04   13.0
    pc_x2                     6.54e-06  2.47e-05  1.35e-06  6.26e-04   12.7
    k4s2_x2                   5.66e-06  2.73e-05  1.58e-06  7.60e-04   13.9
    up2_res                   3.42e-06  2.53e-05  1.25e-06  7.06e-04   14.0
    zins2_res                 6.19e-06  3.60e-05  1.59e-06  7.81e-04   10.8
    zins2_tail                4.80e-06  2.74e-05  1.40e-06  5.94e-04   10.8
    k3s2                      4.03e-06  2.69e-05  1.40e-06  6.81e-04   12.7
    k4s2_pooled               1.06e-05  2.25e-05  3.33e-06  8.63e-04   19.2
    phases_up2                6.56e-06  2.97e-05  3.53e-06  1.01e-03   16.9
    phases_dgrad              3.18e-06  2.45e-05  1.19e-06  5.69e-04   11.6
    k2s2                      2.97e-06  2.35e-05  1.28e-06  5.45e-04   11.6
    k2s2_tail                 4.08e-06  2.53e-05  1.55e-06  7.07e-04   14.0
    plain                     8.29e-06  1.18e-05  1.23e-06  6.14e-04   26.0
    ragged                    8.47e-06  1.26e-05  1.22e-06  5.75e-04   22.8
    ragged_odd_width          8.13e-06  1.02e-05  9.91e-07  4.68e-04   22.9
    low_4x16                  5.06e-06  1.22e-05  1.46e-06  6.51e-04   26.7
    up2                       9.32e-06  1.49e-05  1.63e-06  6.72e-04   22.5
    s2                        5.44e-06  1.34e-05  1.23e-06  6.63e-04   24.7
    k2s2                      6.55e-06  1.41e-05  1.14e-06  5.70e-04   20.2
    virtual_dy_groups2        1.33e-05  1.40e-05  1.34e-06  6.69e-04   23.9
    accumulate                7.92e-06  1.39e-05  1.32e-06  6.32e-04   22.8
    pc16_128                  1.39e-05  1.38e-05  1.52e-06  7.88e-04   28.5
    pc16_64                   1.17e-05  1.29e-05  1.43e-06  6.45e-04   24.9
    pc16_virtual_dy_groups2   1.46e-05  1.44e-05  1.23e-06  6.01e-04   20.8
    pc16_up2                  1.38e-05  1.49e-05  1.40e-06  7.03e-04   23.5
    pc16_up2_virtual_dy       1.82e-05  1.42e-05  1.46e-06  7.35e-04   25.8
    pair_a                    1.44e-05  1.53e-05  1.40e-06  6.43e-04   21.0
    pair_b                    1.08e-05  1.20e-05  1.22e-06  6.42e-04   26.8

e3 is a few times e6 everywhere: the hi*hi instruction, whose +-1 ... +-9 products cancel, costs the small sum it meets a few low bits (as
if the matrix pipe aligned its accumulator to the largest product it adds).  That loss grows with the number of such instructions behind
one output element and is why the weight-gradient operands keep oracle.x3_products.LIVE_PIXELS live pixels: with a dense output gradient
the (8, 64, 64, 48, 64) problem measured e3 = 3.8e-5 on conv_wgrad_x3pc16_kernel (K = 16 per instruction) and 2.3e-5 on
conv_wgrad_x3_kernel (K = 32) next to e0 = 1.4e-5 -- and 1.8e-7 / 3.3e-7 with the same tails and no integers.  A kernel with one matrix
instruction removed or duplicated (scratch builds, one per kernel body) measured e3 = 6.1e-4 ... 1.3e-3 in EVERY case of its family, equal to
the emulation's figure for that variant to two digits (e.g. pc16_128 without mid*mid: 7.78e-4 measured, 7.88e-4 emulated)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check  # noqa: E402
from oracle import x3_products as X  # noqa: E402
from test_x3_gpu import _run_group, dev  # noqa: E402

DEV = "cuda"


def judge(name, got3, got0, e, form, ids, mult=1.0):
    """the assertions of the module docstring; `ids`: the profiling ids of the X3 launches; `mult`: the result is this multiple of the
    reference (accumulate)"""
    ref = e.ref * mult
    scale = e.scale * mult
    e3 = float((got3.detach().cpu().double() - ref).abs().max()) / scale
    e0 = float((got0.detach().cpu().double() - ref).abs().max()) / scale
    t = max(2.0 * e0, 4.0 * e.e6)
    print(f"{name:24s} e3 {e3:.2e}  e0 {e0:.2e}  e6 {e.e6:.2e}  five {e.five_min:.2e}  ratio {e.five_min / t:6.1f}  {' '.join(ids)}")
    assert ids == [form], f"{name}: the launch ran as {ids}, the case is about {form}"
    assert e.five_min >= 5.0 * t, f"{name}: inputs do not discriminate: fp32-MFMA error e0 = {e0:.3e}, e6 = {e.e6:.3e}, smallest five-product error {e.five_min:.3e}"
    assert e3 <= t, f"{name}: X3 error {e3:.3e} > {t:.3e} (fp32-MFMA {e0:.3e}, six-product emulation {e.e6:.3e}, five products {e.five_min:.3e})"


def ran(launch, prefix):
    """run `launch` bracketed by the library's profiler: the ids of the launches whose id contains `prefix`"""
    _ffi.prof_start(prefix)
    try:
        out = launch()
    finally:
        ids = _ffi.prof_stop()
    return out, sorted(ids)


def pack(c, wt, x3):
    """the case's weights [cout][cin][3 or ks][..] through the table-driven pack kernels: pack 0 as they are, 1 the pooled 4x4 kernel,
    2 / 3 the four 2x2 phase kernels"""
    ks_src = wt.shape[2]
    sub = int((lib.ctl_conv_wpack_floats_x3 if x3 else lib.ctl_conv_wpack_floats)(c.cin, c.cout, c.ks))
    nrec = 4 if c.pack in (2, 3) else 1
    table = torch.tensor([[0, z * sub, c.cout, c.cin, c.ks, z, c.cin * ks_src * ks_src, ks_src * ks_src, ks_src, 1, sub, c.pack | (_ffi.PACK_X3 if x3 else 0)]
                          for z in range(nrec)], dtype=torch.int64, device=DEV)
    out = torch.zeros(nrec * sub, device=DEV)
    src = wt.to(DEV).contiguous()
    fn = lib.ctl_pack_weights_x3_batched if x3 else lib.ctl_pack_weights_batched
    check(fn(src.data_ptr(), out.data_ptr(), table.data_ptr(), nrec, sub, ops.stream_ptr()), "pack")
    return out


@pytest.mark.parametrize("c", X.FWD_CASES, ids=[c.name for c in X.FWD_CASES])
def test_forward_forms_form_six_products(c):
    e = X.forward_case(c)
    n, cout = c.n, c.cout
    if c.nsub == 4:
        ho, wo, oh, ow = c.h, c.w, 2 * c.h, 2 * c.w
    elif c.in_mode:
        ho, wo = 2 * c.h, 2 * c.w
        oh, ow = ho, wo
    else:
        ho, wo = (c.h + c.stride - 1) // c.stride, (c.w + c.stride - 1) // c.stride
        oh, ow = ho, wo
    assert tuple(e.ref.shape) == (n, cout, oh, ow)
    kw = dict(n=n, hin=c.h, win=c.w, cin=c.cin, hout=ho, wout=wo, cout=cout, ks=c.ks, stride=c.stride, in_mode=c.in_mode, pro_affine=c.pro)
    if c.nsub == 4:
        kw.update(pad=2 if c.pack == 2 else 0, nsub=4, out_h=oh, out_w=ow, out_sy=2, out_sx=2, out_sub=1)
    g = torch.Generator().manual_seed(7)
    args = {}
    if c.pro == 1:          # BatchNorm apply + LeakyReLU with scale 1, shift 0, slope 1
        kw.update(pro_slope=1.0)
        args.update(pro_scale=dev(torch.ones(c.cin)), pro_shift=dev(torch.zeros(c.cin)))
    elif c.pro == 2:        # the virtual tensor 1 * x + 0 * x2 + 0
        coef = torch.zeros(1, 3, c.cin)
        coef[:, 0] = 1.0
        args.update(pro_scale=dev(coef), x2=dev(torch.randn(n, c.cin, c.h, c.w, generator=g)))
    if c.epi == "res":      # y = conv + 0 * 1 + 0
        kw.update(epi_flags=_ffi.EPI_RES)
        args.update(res=dev(torch.zeros(n, cout, oh, ow)), res_scale=dev(torch.ones(cout)), res_shift=dev(torch.zeros(cout)))
    elif c.epi == "bnbwd":  # y = conv * leaky'(1 * 1 + 0) = conv
        kw.update(epi_flags=_ffi.EPI_STATS | _ffi.EPI_BNBWD, epi_slope=0.2)
        args.update(res=dev(torch.ones(n, cout, oh, ow)), res_scale=dev(torch.ones(1, cout)), res_shift=dev(torch.zeros(1, cout)), want_stats=True)
    elif c.epi == "tail":   # y = conv * leaky'(block output = 1) = conv
        kw.update(epi_flags=_ffi.EPI_STATS | _ffi.EPI_TAILBWD, epi_slope=0.2)
        args.update(res=dev(torch.ones(n, cout, oh, ow)), res2=dev(torch.randn(n, cout, oh, ow, generator=g)), want_stats=True)
    xd = dev(e.x)
    y0 = ops.conv_forward(_ffi.conv_desc(**kw), xd, pack(c, e.w, False), y=ops.empty_nhwc(n, cout, oh, ow, DEV), **args)[0]
    d3 = _ffi.conv_desc(dt=_ffi.DT_X3, **kw)
    (y3, _), ids = ran(lambda: ops.conv_forward(d3, xd, pack(c, e.w, True), y=ops.empty_nhwc(n, cout, oh, ow, DEV), **args), "conv_igemm_x3")
    judge(c.name, y3, y0, e, c.form, ids)


def _wgrad_tensors(c, e):
    """device tensors and the descriptor arguments of a weight-gradient case (identity side inputs)"""
    ho, wo = e.w.shape[2:]
    kw = dict(n=c.n, hin=c.h, win=c.w, cin=c.cin, hout=ho, wout=wo, cout=c.cout, ks=c.ks, stride=c.stride, pad=1 if c.ks == 3 else 0,
              in_mode=_ffi.IN_UP2 if c.up else 0, groups=c.groups, pro_affine=1 if c.pro else 0, pro_slope=1.0 if c.pro else 0.0)
    g = torch.Generator().manual_seed(9)
    sc = dev(torch.ones(c.groups, c.cin)) if c.pro else None
    sh = dev(torch.zeros(c.groups, c.cin)) if c.pro else None
    u = coef = None
    if c.virt:              # the virtual output gradient 1 * dy + 0 * dy2 + 0
        u = dev(torch.randn(c.n, c.cout, ho, wo, generator=g))
        coef = torch.zeros(c.groups, 3, c.cout)
        coef[:, 0] = 1.0
        coef = dev(coef)
    return dict(kw=kw, x=dev(e.x), dy=dev(e.w), sc=sc, sh=sh, u=u, coef=coef)


def _single(m, dt, accumulate=False):
    cin, cout, ks = m["kw"]["cin"], m["kw"]["cout"], m["kw"]["ks"]
    d = _ffi.conv_desc(dt=dt, **m["kw"])
    dw = torch.full((cout, cin, ks, ks), 7.0, device=DEV)
    a = dict(dbias=torch.zeros(cout, device=DEV), pro_scale=m["sc"], pro_shift=m["sh"], dy2=m["u"], dy_coef=m["coef"])
    ops.conv_wgrad(d, m["x"], m["dy"], dw, (cin * ks * ks, ks * ks, ks, 1), **a)
    if accumulate:
        ops.conv_wgrad(d, m["x"], m["dy"], dw, (cin * ks * ks, ks * ks, ks, 1), accumulate=True, **a)
    return dw


@pytest.mark.parametrize("c", X.WGRAD_CASES, ids=[c.name for c in X.WGRAD_CASES])
def test_weight_gradient_forms_form_six_products(c):
    e = X.wgrad_case(c)
    m = _wgrad_tensors(c, e)
    dw0 = _single(m, 0, c.accumulate)
    if c.grouped:           # conv_wgrad_x3pc16_kernel: a grouped launch of one member
        assert lib.ctl_wgrad_group_class(_ffi.desc_ptr(_ffi.conv_desc(dt=_ffi.DT_X3, **m["kw"])), 1 if c.virt else 0) >= 0
        (got, _), ids = ran(lambda: _run_group([m]), "conv_wgrad_x3")
        dw3 = got[0][0]
    else:
        dw3, ids = ran(lambda: _single(m, _ffi.DT_X3, c.accumulate), "conv_wgrad_x3")
    judge(c.name, dw3, dw0, e, c.form, ids, 2.0 if c.accumulate else 1.0)


def test_grouped_launch_of_two_members_forms_six_products():
    """one ctl_conv_wgrad_group launch over two members of different shape: both results are six-product results"""
    es = [X.wgrad_case(c) for c in X.GROUP_PAIR]
    ms = [_wgrad_tensors(c, e) for c, e in zip(X.GROUP_PAIR, es)]
    (got, splits), ids = ran(lambda: _run_group(ms), "conv_wgrad_x3")
    assert len(set(splits)) == 2, splits
    for c, e, m, (dw3, _) in zip(X.GROUP_PAIR, es, ms, got):
        judge(c.name, dw3, _single(m, 0), e, c.form, ids)
