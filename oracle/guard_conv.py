"""What the guard-band GPU tests (tests/test_conv_guard_gpu.py, test_wgrad_guard_gpu.py, test_pack_guard_gpu.py) share: the comparison rule
of each kernel family, copied from the family's own test file so that no new tolerance enters; weight packing through the table-driven pack
kernels; and one guarded ctl_conv_forward_ex launch (buffers sized exactly, poisoned, guards and coverage checked, repeated bit for bit).
The library is loaded when a helper is first called, not on import."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check
from oracle.guarded import Guarded, GuardedCall

DEV = "cuda"
BF = _ffi.DT_BF16
SLOPE = 0.2

RAGGED = [(1, 16, 16, 3, 3), (2, 16, 16, 9, 7), (2, 32, 48, 17, 23), (3, 48, 16, 33, 35), (2, 128, 64, 5, 6), (2, 64, 32, 24, 20)]
PC = [(8, 128, 64, 20, 28), (6, 64, 96, 36, 52)]           # sizes at which the X3 producer / consumer form is picked (tests/test_x3_gpu.py)
NARROW = [(2, 1, 16, 9, 7), (2, 4, 16, 20, 12), (2, 16, 4, 17, 23), (3, 16, 1, 9, 7), (2, 16, 12, 9, 7), (2, 32, 8, 17, 23)]
# Cases of tests/test_kernels_gpu.py, test_x3_gpu.py and test_bf16_gpu.py (h <= 72) kept next to the small ones: the 8x16 and 8x32 pixel
# tiles are only picked once a launch has a few hundred blocks, so the small shapes above all run the 4x16 tile.
# blocks(8x16) = n * ceil(h / 8) * ceil(w / 16) * cout groups >= 384 picks the 8x16 tile, blocks(8x32) >= 512 (at most 768 with 32-channel
# groups) the 8x32 tile (ctl_conv_pick_cfg): the smallest ragged shapes that get there, in place of the files' (16,16,16,64,64),
# (8,64,64,64,64) and (32,16,16,64,64)
TILED = [(8, 16, 48, 30, 62), (8, 64, 64, 46, 62), (8, 16, 48, 58, 66)]
TILED_UP = [(16, 16, 16, 32, 64), (12, 128, 128, 16, 16), (4, 16, 64, 64, 64)]      # in front of a nearest up-sampling (the output is 2h x 2w)
FIRST = [(16, 1, 16, 64, 64), (3, 4, 32, 20, 12)]                                 # <= 4 input channels at the larger tiles
# Channel counts off the 16-grid.  cin 8 / 12: the staging code pads the cin chunk to 16 lanes, and in NHWC the lanes past cin of a pixel
# are the NEXT pixel's channels (a mask that is off by a quad reads real data and multiplies it by the pack's zero weights: only a poisoned,
# exactly-sized buffer shows it).  cout 20 / 24 / 36 / 40: a whole 16-channel output tile plus a partial one, with one (cot odd) and two
# (cot even) cout tiles per block; cout 8 / 12 next to cin 8 / 12; both at once.
OFFGRID = [(2, 8, 16, 9, 7), (2, 12, 32, 17, 23), (3, 8, 8, 20, 12), (2, 12, 12, 9, 7),
           (2, 16, 20, 9, 7), (2, 32, 24, 17, 23), (2, 16, 40, 9, 7), (2, 64, 36, 5, 6), (2, 16, 8, 9, 7),
           (2, 8, 20, 9, 7), (2, 12, 24, 17, 23)]
OFFGRID_EVEN = [(n, ci, co, h + h % 2, w + w % 2) for n, ci, co, h, w in OFFGRID]      # for the stride-2 forms that need even sizes
# cin = 8 at the two larger pixel tiles (the rule above with one cout tile): 16 * 6 * 4 = 384 blocks of 8x16; 16 * 8 * 4 = 512 blocks of 8x32
OFFGRID_TILED = [(16, 8, 8, 48, 64), (16, 8, 8, 64, 128)]
FAMILIES = ["fp32", "x3", "bf16"]


# ------------------------------------------------------------------------------------------------ the families' comparison rules
def rb(t):
    return t.float().to(torch.bfloat16).double()


def f64(t):
    return t.double()


def leaky(x, s):
    return torch.where(x > 0, x, x * s)


def close32(a, b, rel=2e-4, what=""):                      # tests/test_kernels_gpu.py
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    tol = rel * max(float(b.abs().max()), 1e-6) + 1e-7
    err = float((a - b).abs().max())
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e}"      # (a NaN fails this comparison)


def errs(y3, y0, ref, what):                               # tests/test_x3_gpu.py
    ref = ref.detach().double()
    scale = max(float(ref.abs().max()), 1e-30)
    e3 = float((y3.detach().cpu().double() - ref).abs().max()) / scale
    e0 = float((y0.detach().cpu().double() - ref).abs().max()) / scale
    assert e0 <= 2e-4, f"{what}: the fp32 kernel itself is off ({e0:.2e})"
    assert e3 <= max(2.0 * e0, 2e-6), f"{what}: X3 error {e3:.3e} vs fp32-MFMA error {e0:.3e} (relative to max|ref|)"


def close16(a, b, rel, what, bf16_out=False):              # tests/test_bf16_gpu.py
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    tol = rel * max(float(b.abs().max()), 1e-6) + 1e-7
    err = (a - b).abs()
    if bf16_out:
        err = err - b.abs() * 2.0 ** -8
    assert float(err.max()) <= tol, f"{what}: max err {float(err.max()):.3e} > tol {tol:.3e}"


def judge(fam, got, ref, what, pro=False, b16out=False, got32=None):
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite result (a poisoned element was read)"
    if fam == "fp32":
        close32(got, ref, 2e-4, what)
    elif fam == "x3":
        assert got32 is not None, f"{what}: the X3 rule needs the fp32 kernel's result on the same problem"
        errs(got, got32, ref, what)
    else:
        close16(got, ref, 1e-3 if pro else 3e-4, what, b16out)


def _row_ok(got, want, rel, slack, floor, what):
    """|got - want| <= rel * max(max|want|, floor) + slack over one row of per-channel sums"""
    tol = rel * max(float(want.abs().max()), floor) + slack
    err = float((got - want).abs().max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def judge_sums(fam, got, want, what, rule):
    """Statistics partial sums [groups][2][c] (fp64 sum over the partial rows) against the reference sums.  Every BatchNorm group and each
    of its two rows (sum, sum of squares or sum g*u) is held to ITS OWN largest channel, with the figures of the family's file:
      rule "stats" (CTL_EPI_STATS of a forward conv): tests/test_kernels_gpu.py:59-60 close(rel=1e-4) per row; tests/test_x3_gpu.py:117-118
                   1e-4 * max|sum| + 1e-3 and 1e-4 * max(sumsq); tests/test_bf16_gpu.py:69-70 close(2e-4) per row
      rule "bnbwd" (CTL_EPI_BNBWD): tests/test_kernels_gpu.py:185-186 2e-4 * max + 1e-2 per group and row; tests/test_x3_gpu.py:235-237
                   2e-4 * max + 1e-3 per group over both rows together; tests/test_bf16_gpu.py:329-330 2e-3 * max + 5e-2 per group and row
      rule "pro2"  (the BatchNorm-backward prologue with the statistics epilogue alone): the "stats" figures in the fp32 and X3 families;
                   bf16: close(1e-3), the figure tests/test_bf16_gpu.py:313 holds these partials to, per group and row"""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite partial sums"
    assert got.shape == want.shape and got.dim() == 3 and got.shape[1] == 2, (got.shape, want.shape)
    for k in range(got.shape[0]):
        if rule == "bnbwd" and fam == "x3":
            _row_ok(got[k], want[k], 2e-4, 1e-3, 0.0, f"{what} (group {k})")
            continue
        for r in range(2):
            w = f"{what} (group {k}, row {r})"
            if rule == "bnbwd":
                _row_ok(got[k, r], want[k, r], 2e-4 if fam == "fp32" else 2e-3, 1e-2 if fam == "fp32" else 5e-2, 0.0, w)
            elif fam == "bf16":
                _row_ok(got[k, r], want[k, r], 1e-3 if rule == "pro2" else 2e-4, 1e-7, 1e-6, w)
            elif fam == "fp32":
                _row_ok(got[k, r], want[k, r], 1e-4, 1e-7, 1e-6, w)
            else:
                _row_ok(got[k, r], want[k, r], 1e-4, 1e-3 if r == 0 else 0.0, 0.0, w)


# ------------------------------------------------------------------------------------------------ device tensors, packs
def dev(x, b16=False):
    x = x.to(DEV)
    if b16:
        x = x.to(torch.bfloat16)
    return x.contiguous(memory_format=torch.channels_last) if x.dim() == 4 else x.contiguous()


def pack(fam, src, recs):
    """recs: (src_off, cout, cin, ks, flip, strides, mode) per sub-problem -> one packed buffer, sub-problems back to back (zeroed, as
    nets.py hands it to the pack kernels; the pack destinations themselves are the subject of tests/test_pack_guard_gpu.py)"""
    _, cout, cin, ks, _, _, _ = recs[0]
    x3 = fam == "x3"
    sub = int((lib.ctl_conv_wpack_floats_x3 if x3 else lib.ctl_conv_wpack_floats)(cin, cout, ks))
    if recs[0][6] == 4:
        sub = ((cout + 15) // 16) * 3 * 256
    table = torch.tensor([[so, z * sub, co, ci, k, fl, *st, sub, mode | (_ffi.PACK_X3 if x3 else 0)] for z, (so, co, ci, k, fl, st, mode) in enumerate(recs)],
                         dtype=torch.int64, device=DEV)
    out = torch.zeros(len(recs) * sub, device=DEV)
    srcd = src.to(DEV).float().contiguous()
    fn = {"fp32": lib.ctl_pack_weights_batched, "x3": lib.ctl_pack_weights_x3_batched, "bf16": lib.ctl_pack_weights_bf16_batched}[fam]
    check(fn(srcd.data_ptr(), out.data_ptr(), table.data_ptr(), len(recs), sub, ops.stream_ptr()), "pack")
    return out


def pack_fwd(fam, wt):
    co, ci, ks, _ = wt.shape
    return pack(fam, wt, [(0, co, ci, ks, 0, (ci * ks * ks, ks * ks, ks, 1), 0)])


def pack_dgrad(fam, wt):
    co, ci, ks, _ = wt.shape
    return pack(fam, wt, [(0, ci, co, ks, 1, (ks * ks, ci * ks * ks, ks, 1), 0)])


def pack_phases(fam, wt, cout_eff, cin_eff, strides, mode):
    return pack(fam, wt, [(0, cout_eff, cin_eff, 2, z, strides, mode) for z in range(4)])


def x3_ok(cin, cout, ks):
    return ks >= 2 and cin % 16 == 0 and (cout % 16 == 0 or cout in (4, 8, 12))


def chan_ok(cin, cout):
    """the channel counts ctl_conv_pick_cfg serves: cin 1, 4, 8, 12 or a multiple of 16; cout 1 or a multiple of 4"""
    return (cin in (1, 4, 8, 12) or (cin >= 16 and cin % 16 == 0)) and (cout == 1 or cout % 4 == 0)


def refused(kw, names, two=False, wgrad=False):
    """The library must refuse the descriptor before it launches anything: non-zero status and a ctl_last_error that names the channel
    count (`names`: the substrings, e.g. "cin 8" or "got 20").  Every pointer is a buffer large enough for the problem all the same."""
    d = _ffi.conv_desc(**kw)
    dp = _ffi.desc_ptr(d)
    n, cin, cout, ks = int(d["n"]), int(d["cin"]), int(d["cout"]), int(d["ks"])
    px_in, px_out = n * int(d["hin"]) * int(d["win"]), n * int(d["out_h"]) * int(d["out_w"])
    big = torch.zeros(max(px_in * cin, px_out * cout, 4 * ks * ks * (cin + 16) * (cout + 16), 4096) + 4096, device=DEV)
    outs = [torch.zeros_like(big) for _ in range(3)]
    p = big.data_ptr()
    if wgrad:
        rc = lib.ctl_conv_wgrad_ex(dp, p, p, p, p, p if two else None, p if two else None, outs[0].data_ptr(), outs[1].data_ptr(), ops.stream_ptr())
    else:
        rc = lib.ctl_conv_forward_ex(dp, p, p, p, p, p, p, p, p, p, p, outs[0].data_ptr(), outs[1].data_ptr(), None, outs[2].data_ptr() if int(d["pro_affine"]) == 2 else None,
                                     ops.stream_ptr())
    msg = (lib.ctl_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc != 0, f"the library accepted {kw}"
    assert all(not bool(o.any()) for o in outs), f"a refused call wrote to an output ({kw})"
    assert any(s in msg for s in names), f"the refusal does not name the channel count {names}: {msg!r}"
    return msg


def fam_dt(fam, cin, cout, x16=True, y16=True, res16=True):
    """(dt word, x stored as bf16, y stored as bf16, res stored as bf16): bf16-stored tensors have multiples of 16 channels"""
    if fam == "x3":
        return _ffi.DT_X3, False, False, False
    if fam == "fp32":
        return 0, False, False, False
    x16, y16 = x16 and cin % 16 == 0, y16 and cout % 16 == 0
    res16 = res16 and cout % 16 == 0
    return BF | (_ffi.DT_X16 if x16 else 0) | (_ffi.DT_Y16 if y16 else 0) | (_ffi.DT_RES16 if res16 else 0), x16, y16, res16


def fam_cases(shapes, ks, fams=FAMILIES, ok=None):
    """[(n, cin, cout, h, w, family)] for the families that have the form: the X3 family needs cin % 16 == 0, cout % 16 == 0 or 4 / 8 / 12
    and a 2x2 / 3x3 / 4x4 kernel (`ok(family, shape)` narrows further)"""
    return [pytest.param(*s, f, id="-".join(map(str, s)) + "-" + f) for s in shapes for f in fams
            if (f != "x3" or x3_ok(s[1], s[2], ks)) and (ok is None or ok(f, s))]


_STATE = {"again": True}


def each_family(fams, fam):
    """the families of one case in order; the fp32 companion of an X3 case (its result is what errs() compares the X3 error with) runs
    its guarded launches once: the fp32 parameter of the same case repeats them bit for bit"""
    try:
        for f in fams:
            _STATE["again"] = f == fam
            yield f
    finally:
        _STATE["again"] = True


def need(fam, cin, cout, ks):
    assert fam != "x3" or x3_ok(cin, cout, ks), "outside the X3 family (see fam_cases)"
    return ("fp32", "x3") if fam == "x3" else (fam,)


# ------------------------------------------------------------------------------------------------ one guarded launch
def run_conv(kw, x, wp, y_shape, y16=False, y_init=None, want_stats=False, xout_like=None, pool_shape=None, again=True, **a):
    """Steps 1-4 and 6 of a case for one descriptor: returns dict(y, stats [groups][rows][2][cout], xout, pool) as CPU tensors of the first
    run.  y_shape / pool_shape: logical (n, c, h, w); y_init: previous contents of an accumulated y; xout_like: the device x."""
    d = _ffi.conv_desc(**kw)
    dp = _ffi.desc_ptr(d)
    gc = GuardedCall(DEV)
    n, c, h, w = y_shape
    ydt = torch.bfloat16 if y16 else torch.float32
    init = None
    if y_init is not None:
        yi = dev(y_init, y16)
        init = lambda b: b.view(y_shape, channels_last=True).copy_(yi)
    y = gc.out("y", n * c * h * w, ydt, init=init)
    st = xo = pl = None
    if want_stats:
        nst = int(lib.ctl_conv_stats_floats(dp))
        assert nst > 0, "ctl_conv_stats_floats refused the descriptor"
        st = gc.out("stats_partial", nst)
    if xout_like is not None:
        xo = gc.out("xout", xout_like.numel(), xout_like.dtype)
    if pool_shape is not None:
        pl = gc.out("pool", int(np.prod(pool_shape)), ydt)
    p = lambda t: None if t is None else (t.ptr if isinstance(t, Guarded) else t.data_ptr())

    def launch():
        check(lib.ctl_conv_forward_ex(dp, x.data_ptr(), wp.data_ptr(), p(a.get("bias")), p(a.get("pro_scale")), p(a.get("pro_shift")), p(a.get("res")),
                                      p(a.get("res_scale")), p(a.get("res_shift")), p(a.get("res2")), p(a.get("x2")), y.ptr, p(st), p(pl), p(xo),
                                      ops.stream_ptr()), "ctl_conv_forward_ex")

    gc.run(launch)
    out = dict(y=y.view(y_shape, channels_last=True).cpu().contiguous())
    if st is not None:
        groups = max(int(kw.get("groups", 1)), 1)
        rows = int(lib.ctl_conv_stats_blocks(dp))
        assert st.numel == groups * rows * 2 * int(kw["cout"])
        out["stats"] = st.flat().cpu().double().view(groups, rows, 2, int(kw["cout"]))
    if xo is not None:
        out["xout"] = xo.view(xout_like.shape, channels_last=True).cpu().contiguous()
    if pl is not None:
        out["pool"] = pl.view(pool_shape, channels_last=True).cpu().contiguous()
    if again and _STATE["again"]:                                                   # (False: the fp32 companion of an X3 case, whose own parameter repeats it)
        gc.rerun(launch)
    return out


def group_index(n, groups):
    return torch.arange(n) // (n // groups)


def per_group(v, gi):
    """[groups][c] coefficients -> [n, c, 1, 1]"""
    return v[gi].view(len(gi), -1, 1, 1)


def ref_sums(ref, other, gi, groups):
    """[groups][2][c]: (sum ref, sum ref * other) per BatchNorm group"""
    return torch.stack([torch.stack([ref[gi == k].sum((0, 2, 3)), (ref[gi == k] * other[gi == k]).sum((0, 2, 3))]) for k in range(groups)])


def gen_for(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))
