"""The weight-pack kernels behind guard bands.  A packed buffer holds MFMA fragments padded to whole 16-channel tiles (cin_p, cout_p);
the conv kernels read whole fragments.  nets.py re-packs after every optimizer step into one buffer it zeroed once, so the result must
not depend on what the destination held: here the destination is a Guarded of exactly ctl_conv_wpack_floats(_x3) floats filled with NaN
bits, and the packed weights are then consumed by a conv of the matching family on a (2, cin, cout, 9, 7) problem -- a fragment element
the pack left alone and the conv reads arrives in the result as a NaN.

What each layout owns (include/ctl_hip.h): the fp32 and X3 layouts fill the whole destination; the bf16 layout fills the first
ceil(taps / 2) of every `taps` fragments and neither writes nor reads the rest.  Single records, and three records back to back at
their dst_off with poisoned gaps between them."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, ops  # noqa: E402
from cooperative_training_and_latent_space_data_augmentation_amd._ffi import lib, check  # noqa: E402
from oracle.guarded import GuardedCall  # noqa: E402
from oracle.guard_conv import DEV, FAMILIES, chan_ok, dev, each_family, f64, fam_dt, gen_for, judge, rb, refused, run_conv, x3_ok  # noqa: E402

SHAPES = [(16, 16, 3), (48, 32, 3), (4, 16, 3), (1, 16, 1), (16, 1, 3), (16, 4, 3), (12, 16, 3), (32, 16, 2), (16, 16, 4), (64, 128, 1)]      # cout, cin, ks
# cin 8 / 12: the padded cin chunk the conv kernels read as zeros; cout 20 / 24: a whole cout tile and a partial one
SHAPES += [(16, 8, 3), (8, 16, 3), (8, 8, 3), (16, 12, 3), (12, 12, 3), (20, 16, 3), (24, 32, 3), (8, 8, 2), (8, 8, 4), (8, 16, 1), (20, 8, 3)]
N, H, W = 2, 9, 7
GAP = 64                                                      # poisoned floats between two records of one destination
PACK_FN = {"fp32": "ctl_pack_weights_batched", "x3": "ctl_pack_weights_x3_batched", "bf16": "ctl_pack_weights_bf16_batched"}


def sub_floats(fam, cout, cin, ks, mode=0):
    if mode == 4:
        return ((cout + 15) // 16) * 3 * 256
    return int((lib.ctl_conv_wpack_floats_x3 if fam == "x3" else lib.ctl_conv_wpack_floats)(cin, cout, ks))


def owned_floats(fam, cout, cin, ks, mode=0):
    """floats of one record's destination that its pack kernel fills"""
    sub = sub_floats(fam, cout, cin, ks, mode)
    if fam == "bf16":
        return sub // (ks * ks) * ((ks * ks + 1) // 2)
    return sub


def guarded_pack(fam, srcs, recs, gap=0, single_entry=False):
    """recs: (src index, src_off, cout, cin, ks, flip, strides, mode); record k lands at k * (sub + gap).  Returns (Guarded, [float offsets]).
    The destination is exactly the records' floats (+ the gaps); guards, the gaps and the owned part of every record are checked, and a
    second run over a re-poisoned destination must give the same bits."""
    _, _, cout, cin, ks, _, _, mode = recs[0]
    sub = sub_floats(fam, cout, cin, ks, mode)
    own = owned_floats(fam, cout, cin, ks, mode)
    offs = [k * (sub + gap) for k in range(len(recs))]
    gc = GuardedCall(DEV)
    dst = gc.out("wpack", offs[-1] + sub, written=False)
    src = torch.cat([s.to(DEV).float().reshape(-1) for s in srcs])
    soff, o = [], 0
    for s in srcs:
        soff.append(o)
        o += s.numel()
    table = torch.tensor([[soff[si] + so, offs[k], co, ci, kk, fl, *st, sub, md | (_ffi.PACK_X3 if fam == "x3" else 0)]
                          for k, (si, so, co, ci, kk, fl, st, md) in enumerate(recs)], dtype=torch.int64, device=DEV)

    def launch():
        if single_entry:
            si, so, co, ci, kk, fl, st, md = recs[0]
            check(lib.ctl_pack_weights(src.data_ptr() + 4 * (soff[si] + so), dst.ptr, co, ci, kk, *[int(v) for v in st], int(fl), ops.stream_ptr()), "ctl_pack_weights")
        else:
            check(getattr(lib, PACK_FN[fam])(src.data_ptr(), dst.ptr, table.data_ptr(), len(recs), sub, ops.stream_ptr()), PACK_FN[fam])

    def owned_and_gaps():
        bits = dst.bits()
        for k, off in enumerate(offs):
            left = torch.nonzero(bits[off:off + own] == 0x7FC5A5A5).flatten()
            assert left.numel() == 0, f"{fam} record {k}: {int(left.numel())} of the {own} floats the layout owns were not written, first {left[:8].tolist()}"
            if k + 1 < len(offs):
                assert bool((bits[off + sub:offs[k + 1]] == 0x7FC5A5A5).all()), f"{fam} record {k}: the pack wrote into the gap behind its destination"
            if own < sub:
                assert bool((bits[off + own:off + sub] == 0x7FC5A5A5).all()), f"{fam} record {k}: wrote beyond the fragments the bf16 layout owns"

    gc.run(launch)
    owned_and_gaps()
    gc.rerun(launch)
    owned_and_gaps()
    return dst, offs


class _At:
    """a packed record inside a guarded destination, as run_conv takes a weight buffer"""

    def __init__(self, dst, off):
        self.p = dst.ptr + 4 * off

    def data_ptr(self):
        return self.p


def conv_kw(cout, cin, ks, dt, **extra):
    if ks in (1, 3):
        kw = dict(n=N, hin=H, win=W, cin=cin, hout=H, wout=W, cout=cout, ks=ks, dt=dt)
    else:                                                     # 2x2 stride 2 pad 0 / 4x4 stride 2 pad 1 on the 9 x 7 input
        kw = dict(n=N, hin=H, win=W, cin=cin, hout=4, wout=3, cout=cout, ks=ks, stride=2, pad=0 if ks == 2 else 1, dt=dt)
    kw.update(extra)
    return kw


def ref_conv(x, wt, ks, q):
    if ks in (1, 3):
        return F.conv2d(q(x), q(wt), padding=ks // 2)
    return F.conv2d(q(x), q(wt), stride=2, padding=0 if ks == 2 else 1)


def consume(fam, wbuf, cout, cin, ks, x0, wt, what, got32=None, **extra):
    dt, x16, y16, _ = fam_dt(fam, cin, cout)
    q = rb if fam == "bf16" else f64
    x = x0.to(torch.bfloat16).float() if x16 else x0
    kw = conv_kw(cout, cin, ks, dt, **extra)
    xd = dev(x, x16) if cin > 1 else x.to(DEV).contiguous()
    o = run_conv(kw, xd, wbuf, (N, cout, kw["hout"], kw["wout"]), y16)
    judge(fam, o["y"], ref_conv(x, wt, ks, q), what, b16out=y16, got32=got32)
    return o["y"]


def fam_ok(fam, cout, cin, ks):
    return fam != "x3" or x3_ok(cin, cout, ks)


def pack_cases(shapes, ks=None):
    """(cout, cin[, ks], family) for the families whose layout exists for the shape"""
    return [pytest.param(*s, f, id="-".join(map(str, s)) + "-" + f) for s in shapes for f in FAMILIES if fam_ok(f, s[0], s[1], ks or s[2])]


@pytest.mark.parametrize("cout,cin,ks,fam", pack_cases(SHAPES))
def test_pack_mode0_single_and_three_records(cout, cin, ks, fam):
    """OIHW forward weights (mode 0, and flipped / transposed as the data gradient takes them): one record, then three records of three
    weight tensors back to back with poisoned gaps; every packed record is consumed by a conv"""
    g = gen_for(cout, cin, ks, 1)
    x0 = torch.randn(N, cin, H, W, generator=g)
    wts = [torch.randn(cout, cin, ks, ks, generator=g) * 0.3 for _ in range(3)]
    st = (cin * ks * ks, ks * ks, ks, 1)
    y32 = {}
    for f in each_family(("fp32", "x3") if fam == "x3" else (fam,), fam):
        dst, offs = guarded_pack(f, wts[:1], [(0, 0, cout, cin, ks, 0, st, 0)])
        y = consume(f, _At(dst, 0), cout, cin, ks, x0, wts[0], f"{f} single record", y32.get("one"))
        if f == "fp32":
            y32["one"] = y
        dst3, offs3 = guarded_pack(f, wts, [(k, 0, cout, cin, ks, 0, st, 0) for k in range(3)], gap=GAP)
        for k in range(3):
            y = consume(f, _At(dst3, offs3[k]), cout, cin, ks, x0, wts[k], f"{f} record {k} of three", y32.get(k))
            if f == "fp32":
                y32[k] = y
    # the data-gradient orientation (flip, transposed strides): cout_eff = cin, cin_eff = cout
    if ks == 3 and cin > 1 and not chan_ok(cout, cin):          # (cout 20 / 24 is no input channel count: no conv takes such a pack)
        refused(conv_kw(cin, cout, ks, 0), [f"got {cout}"])
    elif ks == 3 and fam_ok(fam, cin, cout, ks) and cin > 1:
        xg = torch.randn(N, cout, H, W, generator=g)
        yd = None
        for f in each_family(("fp32", "x3") if fam == "x3" else (fam,), fam):
            dst, _ = guarded_pack(f, wts[:1], [(0, 0, cin, cout, ks, 1, (ks * ks, cin * ks * ks, ks, 1), 0)])
            dt, x16, y16, _ = fam_dt(f, cout, cin)
            q = rb if f == "bf16" else f64
            xx = xg.to(torch.bfloat16).float() if x16 else xg
            o = run_conv(conv_kw(cin, cout, ks, dt), dev(xx, x16), _At(dst, 0), (N, cin, H, W), y16)
            judge(f, o["y"], F.conv_transpose2d(q(xx), q(wts[0]), padding=1), f"{f} data-gradient pack", b16out=y16, got32=yd)
            if f == "fp32":
                yd = o["y"]


@pytest.mark.parametrize("cout,cin,ks", SHAPES)
def test_pack_weights_single_entry_point(cout, cin, ks):
    """ctl_pack_weights (one effective conv, fp32 layout)"""
    g = gen_for(cout, cin, ks, 2)
    x0 = torch.randn(N, cin, H, W, generator=g)
    wt = torch.randn(cout, cin, ks, ks, generator=g) * 0.3
    dst, _ = guarded_pack("fp32", [wt], [(0, 0, cout, cin, ks, 0, (cin * ks * ks, ks * ks, ks, 1), 0)], single_entry=True)
    dst.check_written()
    consume("fp32", _At(dst, 0), cout, cin, ks, x0, wt, "ctl_pack_weights")


@pytest.mark.parametrize("cout,cin,fam", pack_cases([(16, 16), (48, 32), (4, 16), (12, 16), (64, 128), (16, 8), (20, 16)], 4))
def test_pack_mode1_pooled_4x4_from_3x3(cout, cin, fam):
    """mode 1: the 4x4 stride-2 kernel of sumpool2(conv3x3^T(.)), K[u] = sum of the 3x3 taps W[a + 2 - u] over a in {0, 1} per axis,
    formed inside the pack from a 3x3 source read with the record's strides"""
    g = gen_for(cout, cin, 4, 3)
    x0 = torch.randn(N, cin, H, W, generator=g)
    w3 = torch.randn(cout, cin, 3, 3, generator=g) * 0.2     # read as W[co][ci][kh][kw]
    K = torch.zeros(cout, cin, 4, 4)
    for a in range(2):
        for b in range(2):
            for kh in range(3):
                for kw_ in range(3):
                    K[:, :, a + 2 - kh, b + 2 - kw_] += w3[:, :, kh, kw_]
    y32 = None
    for f in each_family(("fp32", "x3") if fam == "x3" else (fam,), fam):
        dst, _ = guarded_pack(f, [w3], [(0, 0, cout, cin, 4, 0, (cin * 9, 9, 3, 1), 1)])
        y = consume(f, _At(dst, 0), cout, cin, 4, x0, K, f"{f} mode 1", y32)
        if f == "fp32":
            y32 = y


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("cout,cin,fam", pack_cases([(16, 16), (32, 16), (48, 32), (4, 16), (16, 8), (20, 16)], 2))
def test_pack_modes_2_and_3_phase_records(cout, cin, fam, mode):
    """modes 2 / 3: the four 2x2 phase kernels of a 3x3 conv on a nearest-upsampled input / of the data gradient of a stride-2 3x3 conv,
    four records back to back (the conv takes them as its four sub-problems)"""
    g = gen_for(cout, cin, mode, 4)
    x0 = torch.randn(N, cin, H, W, generator=g)
    w3 = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    y32 = None
    for f in each_family(("fp32", "x3") if fam == "x3" else (fam,), fam):
        dst, offs = guarded_pack(f, [w3], [(0, 0, cout, cin, 2, z, (cin * 9, 9, 3, 1), mode) for z in range(4)])
        dt, x16, y16, _ = fam_dt(f, cin, cout)
        q = rb if f == "bf16" else f64
        x = x0.to(torch.bfloat16).float() if x16 else x0
        kw = dict(n=N, hin=H, win=W, cin=cin, hout=H, wout=W, cout=cout, ks=2, stride=1, pad=2 if mode == 2 else 0, nsub=4, out_h=2 * H, out_w=2 * W,
                  out_sy=2, out_sx=2, out_sub=1, dt=dt)
        o = run_conv(kw, dev(x, x16), _At(dst, 0), (N, cout, 2 * H, 2 * W), y16)
        # reference from the definition of the phase kernels (ctl_conv.hip): phase (a, b), tap (kh, kw) of the 2x2 kernel
        ref = torch.zeros(N, cout, 2 * H, 2 * W, dtype=torch.float64)
        for a in range(2):
            for b in range(2):
                k = torch.zeros(cout, cin, 2, 2)
                for kh in range(2):
                    for kw_ in range(2):
                        if mode == 2:
                            hs = range(0, (1 if a else 0) + 1) if kh == 0 else range(2 if a else 1, 3)
                            ws = range(0, (1 if b else 0) + 1) if kw_ == 0 else range(2 if b else 1, 3)
                            for sh in hs:
                                for sw in ws:
                                    k[:, :, kh, kw_] += w3[:, :, sh, sw]
                        else:
                            sh = (2 if kh == 0 else 0) if a else (1 if kh == 0 else -1)
                            sw = (2 if kw_ == 0 else 0) if b else (1 if kw_ == 0 else -1)
                            if sh >= 0 and sw >= 0:
                                k[:, :, kh, kw_] = w3[:, :, sh, sw]
                if mode == 2:      # y[2i+a] = tap0 * x[i + a - 1] + tap1 * x[i + a]
                    xp = F.pad(q(x), (1, 1, 1, 1))
                    ref[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], q(k))
                else:              # dx[2i+a] = tap0 * dy[i] + tap1 * dy[i + 1]
                    xp = F.pad(q(x), (0, 1, 0, 1))
                    ref[:, :, a::2, b::2] = F.conv2d(xp, q(k))
        judge(f, o["y"], ref, f"{f} phase records mode {mode}", b16out=y16, got32=y32)
        if f == "fp32":
            y32 = o["y"]


@pytest.mark.parametrize("cout,cin", [(16, 1), (16, 4), (48, 4), (4, 4)])
def test_pack_mode4_k_packed_first_layer(cout, cin):
    """mode 4: 3x3 taps packed into the MFMA k dimension for inputs with <= 4 channels (fp32 layout, CTL_IN_C4 conv); single and three records"""
    g = gen_for(cout, cin, 4, 5)
    x0 = torch.randn(N, cin, H, W, generator=g)
    wts = [torch.randn(cout, cin, 3, 3, generator=g) * 0.3 for _ in range(3)]
    st = (cin * 9, 9, 3, 1)
    dst, _ = guarded_pack("fp32", wts[:1], [(0, 0, cout, cin, 3, 0, st, 4)])
    dst.check_written()
    consume("fp32", _At(dst, 0), cout, cin, 3, x0, wts[0], "mode 4 single record", in_mode=_ffi.IN_C4)
    dst3, offs3 = guarded_pack("fp32", wts, [(k, 0, cout, cin, 3, 0, st, 4) for k in range(3)], gap=GAP)
    for k in range(3):
        consume("fp32", _At(dst3, offs3[k]), cout, cin, 3, x0, wts[k], f"mode 4 record {k} of three", in_mode=_ffi.IN_C4)
