"""The adversarial-augmentation kernels (csrc/ctl_adv.hip) through the C ABI against the float64 host statement of adversarial.py; every
buffer a kernel writes sits in a guard-banded, poisoned buffer (oracle/guarded.py) and every launch is repeated for the same bits.

Bounds, from the number formats.  The inputs are fp32, exact in fp64; the kernels and the statement both work in fp64 and every output is
rounded to fp32 once.  With u = 2^-24 (half an fp32 spacing, relative) and e = 2^-53:
  f, x'    one fp32 rounding, u |ref|, plus a few fp64 units: a basis weight is a cubic in t (at most 8 operations), a term of S the
           product of two weights and theta, the sum has 16 terms -- |dS| <= 48 e max|theta| on each side, which exp turns into a relative
           error, plus 2 e for exp itself and 2 e for the product with x:  REL_F = (96 max|theta| + 16) e  covers both sides.
  dx       g f rounded once: u |ref| + REL_F |ref|.
  dtheta   an ordered sum of the terms  My[y,a] Mx[x,b] f(y,x) g_c(y,x) x_c(y,x)  over the pixels of the clipped 4s x 4s support and the
           channels, n_terms = min(4s, H) min(4s, W) C of them, rounded once:  u |ref| + 2 (n_terms + 8) e sum|terms|;  the sum of the
           absolute terms is evaluated by the statement per case (the adjoint applied to f sum_c |g_c x_c|).  The few e of f and of the
           weights in each term are the "+ 8".
  unit     scale g / norm rounded once: u |ref|, plus the relative error of the norm -- 'l2' / 'rms': a sum of m squares,
           2 (m + 8) e relative (the square root halves it; both sides are counted), 'linf': exact -- plus 8 e for the division and the
           product.  A sample whose norm is 0 or not finite gives exact zeros.
The largest error seen per output is printed as a fraction of its bound (README, "adversarial input augmentation")."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.guarded import GuardedCall  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, adversarial as A, ops  # noqa: E402

DEV = "cuda"
lib = _ffi.lib
check = _ffi.check
U, E53 = 2.0 ** -24, 2.0 ** -53
PLANES = [(1, 1), (5, 7), (16, 16), (31, 65), (33, 64)]
SPACINGS = [2, 4, 5, 8, 32]                       # 32 (and 8, 5 on the small planes) is larger than the plane
CHANNELS = [1, 4, 16]
THETAS = ["random", "zero", "saturated"]
LOG13 = math.log(1.3)
WORST = {}


def sp():
    return torch.cuda.current_stream().cuda_stream


def worst(key, frac):
    WORST[key] = max(WORST.get(key, 0.0), float(frac))


def make_case(n, c, h, w, s, theta_kind, zero_bg, one_hot, seed):
    """(x, theta, g) fp32 on the host; x and g logical [n,C,H,W] with NHWC memory"""
    gen = torch.Generator().manual_seed(seed)
    gh, gw = A.bias_grid(h, w, s)
    x = torch.randn(n, h, w, c, generator=gen)
    if zero_bg:                                    # an exactly-zero background
        x[:, :h // 2 + 1, :w // 2 + 1] = 0.0
    if theta_kind == "random":
        theta = (torch.rand(n, gh, gw, generator=gen) * 2.0 - 1.0) * 0.26
    elif theta_kind == "zero":
        theta = torch.zeros(n, gh, gw)
    else:                                          # saturated at +- log(1.3)
        theta = torch.where(torch.rand(n, gh, gw, generator=gen) < 0.5, -1.0, 1.0) * float(torch.tensor(LOG13, dtype=torch.float32))
    if one_hot:
        g = torch.zeros(n, h, w, c)
        g[n - 1, h - 1 - (h - 1) // 3, (w - 1) // 2, c - 1] = 1.5
        x[n - 1, h - 1 - (h - 1) // 3, (w - 1) // 2, c - 1] = 0.75          # (not in the zero background)
    else:
        g = torch.randn(n, h, w, c, generator=gen)
    return x.permute(0, 3, 1, 2), theta, g.permute(0, 3, 1, 2)


def run_bias(xd, td, gd, s, with_f=True, with_dx=True, ws_offset=0, rerun=True):
    """guarded forward + backward through the C ABI -> (x', f, dtheta, dx) on the host"""
    n, c, h, w = xd.shape
    gh, gw = A.bias_grid(h, w, s)
    gc = GuardedCall(DEV)
    y = gc.out("y", xd.numel())
    f = gc.out("f", n * h * w) if with_f else None
    need = lib.ctl_adv_bias_ws_bytes(n, h, w, s)
    assert need == 8 * n * gw * h
    ws = gc.out("ws", need // 8 + (1 if ws_offset else 0), torch.float64, written=not ws_offset)
    dth = gc.out("dtheta", n * gh * gw)
    dx = gc.out("dx", xd.numel()) if with_dx else None

    def launch():
        check(lib.ctl_adv_bias_fwd(xd.data_ptr(), td.data_ptr(), n, h, w, c, s, gh, gw, y.ptr, f.ptr if f else None, sp()), "fwd")
        check(lib.ctl_adv_bias_bwd(gd.data_ptr(), xd.data_ptr(), td.data_ptr(), n, h, w, c, s, gh, gw, ws.ptr + ws_offset, need, dth.ptr,
                                   dx.ptr if dx else None, sp()), "bwd")

    before = lib.ctl_launch_count()
    gc.run(launch)
    assert lib.ctl_launch_count() - before == 1 + 2                  # ONE forward launch, TWO backward launches
    if rerun:
        gc.rerun(launch)                                             # guards, every element written, the same bits again
    cl = lambda b: b.view((n, c, h, w), channels_last=True).cpu().clone()      # noqa: E731
    return (cl(y), f.view((n, h, w)).cpu().clone() if f else None, dth.view((n, gh, gw)).cpu().clone(), cl(dx) if dx else None)


def check_bias(tag, x, theta, g, s, got):
    y, f, dth, dx = got
    n, c, h, w = x.shape
    yr, fr = A.bias_field_host(x, theta, s)
    dtr, dxr = A.bias_field_grad_host(g, x, theta, s)
    rel_f = (96.0 * float(theta.abs().max()) + 16.0) * E53
    My, Mx = A.bias_weights(h, s), A.bias_weights(w, s)
    terms = torch.einsum("ya,nyx,xb->nab", My, fr * (g.double() * x.double()).abs().sum(1), Mx)
    n_terms = min(4 * s, h) * min(4 * s, w) * c
    outs = [("x'", y, yr, U * yr.abs() + rel_f * yr.abs()), ("dtheta", dth, dtr, U * dtr.abs() + 2.0 * (n_terms + 8) * E53 * terms)]
    if f is not None:
        outs.append(("f", f, fr, U * fr + rel_f * fr))
    if dx is not None:
        outs.append(("dx", dx, dxr, U * dxr.abs() + rel_f * dxr.abs()))
    for name, got_t, ref, bound in outs:
        assert got_t.dtype == torch.float32 and bool(torch.isfinite(got_t).all()), (tag, name)
        err = (got_t.double() - ref).abs()
        ok = err <= bound
        frac = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
        worst(name, frac)
        assert bool(ok.all()), (tag, name, frac, float(err.max()))
    empty = ((My == 0).all(0).view(-1, 1) | (Mx == 0).all(0).view(1, -1)).expand_as(dth)
    assert bool((dth[empty] == 0).all()), (tag, "a control point with an empty support")
    return dtr


@pytest.mark.parametrize("s", SPACINGS)
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: "x".join(map(str, p)))
def test_bias_kernels_match_the_host_statement(plane, s):
    h, w = plane
    pi, si = PLANES.index(plane), SPACINGS.index(s)
    k = 0
    for n in (1, 3):
        for ci, c in enumerate(CHANNELS):
            for ti, theta_kind in enumerate(THETAS):
                k += 1
                zero_bg, one_hot = bool((ti + ci + n + pi) % 2), bool((k + si + pi) % 3 == 0)      # every pair occurs over the planes and spacings
                x, theta, g = make_case(n, c, h, w, s, theta_kind, zero_bg, one_hot, 1000 * c + 10 * h + w + s + n + 7 * ti)
                xd, td, gd = x.to(DEV), theta.to(DEV), g.to(DEV)
                assert xd.permute(0, 2, 3, 1).is_contiguous() and gd.permute(0, 2, 3, 1).is_contiguous()
                tag = (plane, s, n, c, theta_kind, zero_bg, one_hot)
                got = run_bias(xd, td, gd, s, with_f=bool(k % 2), with_dx=bool((k // 2) % 2), rerun=ti == 0)
                check_bias(tag, x, theta, g, s, got)
                if theta_kind == "zero":                                 # f = exp(0): the image itself
                    assert torch.equal(got[0], x)
                if one_hot:                                              # non-zero only on that pixel's 4 x 4 control points
                    py, px = h - 1 - (h - 1) // 3, (w - 1) // 2
                    box = torch.zeros_like(got[2], dtype=torch.bool)
                    box[n - 1, py // s:py // s + 4, px // s:px // s + 4] = True
                    assert bool((got[2][~box] == 0).all()) and bool((got[2][box] != 0).any()), tag
    print("adv-error bias (largest error / bound): " + "; ".join(f"{k}: {v:.3f}" for k, v in WORST.items()))


def test_bias_large_plane_rows_wider_than_a_block_and_a_capped_grid():
    """520 x 700 x 3 samples: rows of more than one block's threads, more pixels than the forward's capped grid covers in one sweep"""
    n, c, h, w, s = 3, 1, 520, 700, 32
    x, theta, g = make_case(n, c, h, w, s, "random", True, False, 5)
    got = run_bias(x.to(DEV), theta.to(DEV), g.to(DEV), s, rerun=False)
    check_bias("large", x, theta, g, s, got)
    print("adv-error bias, large plane (largest error / bound): " + "; ".join(f"{k}: {v:.3f}" for k, v in WORST.items()))


def run_unit(gd, norm, scale, rerun=True):
    n = gd.shape[0]
    m = gd.numel() // n
    gc = GuardedCall(DEV)
    need = lib.ctl_adv_unit_scale_ws_bytes(n, m)
    assert need == 8 * n * -(-m // 16384)
    ws = gc.out("ws", need // 8, torch.float64)
    out = gc.out("out", gd.numel())

    def launch():
        check(lib.ctl_adv_unit_scale(gd.data_ptr(), n, m, ops.ADV_NORMS[norm], scale, ws.ptr, need, out.ptr, sp()), "unit_scale")

    before = lib.ctl_launch_count()
    gc.run(launch)
    assert lib.ctl_launch_count() - before == 2
    if rerun:
        gc.rerun(launch)
    return out.flat().cpu().clone().view(n, m)


@pytest.mark.parametrize("norm", ["l2", "rms", "linf"])
def test_unit_scale_matches_the_host_statement(norm):
    scale = 0.05 if norm == "rms" else LOG13
    for n, m in ((1, 1), (3, 121), (5, 16384), (5, 16385), (4, 3 * 16384 + 5), (2, (1 << 20) + 77)):
        gen = torch.Generator().manual_seed(n * 31 + m)
        g = torch.randn(n, m, generator=gen) * 1e-3
        bad = {}
        if n >= 3:
            g[1] = 0.0
            bad[1] = "zero"
        if n >= 4:
            g[2, m // 2] = float("nan")
            bad[2] = "nan"
        if n >= 5:
            g[3, m - 1] = float("-inf")
            bad[3] = "inf"
        got = run_unit(g.to(DEV), norm, scale, rerun=m < (1 << 20))
        ref = A.unit_scale_host(g, scale, norm)
        rel = U + (0.0 if norm == "linf" else 2.0 * (m + 8) * E53) + 8.0 * E53
        for k in range(n):
            if k in bad:
                assert bool((got[k] == 0).all()), (norm, n, m, bad[k])
                continue
            err = (got[k].double() - ref[k]).abs()
            bound = rel * ref[k].abs() + 2.0 ** -150
            worst("unit " + norm, float((err / bound).max()))
            assert bool((err <= bound).all()), (norm, n, m, k, float((err / bound).max()))
            r = A._norm(got[k:k + 1].double(), norm)
            assert abs(float(r) - scale) <= scale * (2.0 * U + rel), (norm, n, m, k, float(r))      # the radius itself
    print("adv-error unit step (largest error / bound): " + "; ".join(f"{k}: {v:.3f}" for k, v in WORST.items() if k.startswith("unit")))


def test_same_bits_in_a_graph_replay_at_every_alignment_and_with_an_offset_workspace():
    n, c, h, w, s = 3, 4, 33, 34, 5
    x, theta, g = make_case(n, c, h, w, s, "random", False, False, 77)
    xd, td, gd = x.to(DEV), theta.to(DEV), g.to(DEV)
    y1, f1 = ops.adv_bias_fwd(xd, td, s, with_field=True)
    dt1, dx1 = ops.adv_bias_bwd(gd, xd, td, s)
    u1 = ops.adv_unit_scale(dt1, LOG13, "linf")
    v1 = ops.adv_unit_scale(dx1, 0.05, "rms")
    assert v1.shape == dx1.shape and v1.stride() == dx1.stride()
    assert torch.equal(ops.adv_bias_fwd(xd, td, s), y1) and ops.adv_bias_bwd(gd, xd, td, s, need_dx=False)[1] is None
    # the guarded C-ABI call gives the wrappers' bits, with the workspace on its natural alignment and 8 bytes off it
    for off in (0, 8):
        gy, gf, gdt, gdx = run_bias(xd, td, gd, s, ws_offset=off)
        assert torch.equal(gy, y1.cpu()) and torch.equal(gf, f1.cpu()) and torch.equal(gdt, dt1.cpu()) and torch.equal(gdx, dx1.cpu()), off
    # tensors 4 bytes off the 16-byte grid
    flat = [torch.empty(xd.numel() + 1, device=DEV) for _ in range(2)] + [torch.empty(td.numel() + 1, device=DEV)]
    xo, go = (fl[1:].view(n, h, w, c).permute(0, 3, 1, 2) for fl in flat[:2])
    to = flat[2][1:].view_as(td)
    xo.copy_(xd), go.copy_(gd), to.copy_(td)
    assert xo.data_ptr() % 16 == 4 and to.data_ptr() % 16 == 4
    y3, f3 = ops.adv_bias_fwd(xo, to, s, with_field=True)
    dt3, dx3 = ops.adv_bias_bwd(go, xo, to, s)
    assert torch.equal(y3, y1) and torch.equal(f3, f1) and torch.equal(dt3, dt1) and torch.equal(dx3, dx1)
    assert torch.equal(ops.adv_unit_scale(flat[2][1:].view_as(td).copy_(dt1), LOG13, "linf"), u1)
    # a graph replay of forward, backward and both unit steps
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        yg, fg = ops.adv_bias_fwd(xd, td, s, with_field=True)
        dtg, dxg = ops.adv_bias_bwd(gd, xd, td, s)
        ug = ops.adv_unit_scale(dtg, LOG13, "linf")
        vg = ops.adv_unit_scale(dxg, 0.05, "rms")
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in (yg, fg, dtg, dxg, ug, vg):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, y1) and torch.equal(fg, f1) and torch.equal(dtg, dt1) and torch.equal(dxg, dx1)
        assert torch.equal(ug, u1) and torch.equal(vg, v1)
